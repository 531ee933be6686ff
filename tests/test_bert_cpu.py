"""CPU suite of FrozenBERTEmbedder: the state_dict surface, the WordPiece tokenizer and the text splitting against the reference's
recorded behaviour (tests/golden/bert.npz + bert_surface.json, make_golden_bert.py), the model-directory readers, and every refusal.
Nothing here launches a kernel."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import bert_ref
from util import GOLD, LDM_SMALL, AE_SMALL, gold

TINY_DIR = os.path.join(GOLD, "bert_tiny")


def surf():
    with open(os.path.join(GOLD, "bert_surface.json")) as f:
        return json.load(f)


def tiny_cfg(**over):
    with open(os.path.join(TINY_DIR, "config.json")) as f:
        return dict(json.load(f), **over)


def make_dir(dst, fmt="safetensors", cfg=None, sd=None, prefix="bert_tiny."):
    """a complete model directory: the committed config / vocab / tokenizer config plus seed-recipe weights in the given format"""
    os.makedirs(dst, exist_ok=True)
    for name in ("vocab.txt", "tokenizer_config.json"):
        shutil.copy(os.path.join(TINY_DIR, name), dst)
    cfg = tiny_cfg() if cfg is None else cfg
    with open(os.path.join(dst, "config.json"), "w") as f:
        json.dump(cfg, f)
    sd = bert_ref.seeded_state_dict(cfg, prefix) if sd is None else sd
    if fmt == "safetensors":
        bert_ref.write_safetensors(os.path.join(dst, "model.safetensors"), sd)
    else:
        torch.save(sd, os.path.join(dst, "pytorch_model.bin"))
    return str(dst)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    return make_dir(tmp_path_factory.mktemp("bert_tiny"))


def bert_ldm(ckpt_path, key="crossattn", timesteps=999):
    """The LatentDiffusion of make_golden_bert.py's chain: small SpatialTransformer UNet (context 64), FrozenBERTEmbedder cond stage."""
    from jointimagegeneration_amd.ldm import LatentDiffusion
    unet = dict(LDM_SMALL, in_channels=4, use_spatial_transformer=True, transformer_depth=1, context_dim=64)
    cfg_ae = dict(target="ldm.models.autoencoder.AutoencoderKL", params=dict(embed_dim=4, dims=2, ddconfig=dict(AE_SMALL), lossconfig=dict(target="torch.nn.Identity")))
    m = LatentDiffusion(first_stage_config=cfg_ae, cond_stage_config=dict(target="ldm.modules.encoders.modules.FrozenBERTEmbedder",
                                                                          params=dict(ckpt_path=ckpt_path, device="cpu")),
                        unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=unet), conditioning_key=key,
                        linear_start=0.0015, linear_end=0.0195, timesteps=timesteps, image_size=8, channels=4, dims=2,
                        first_stage_key="image", cond_stage_key="caption", num_timesteps_cond=1)
    m.cond_stage_model.bert_max_length = surf()["n_tok"]
    return m


# ------------------------------------------------------------------------------------------------ surface, paths
def test_state_dict_surface_equals_both_reference_copies(tiny):
    from jointimagegeneration_amd import cond
    s = surf()
    m = cond.FrozenBERTEmbedder(tiny, device="cpu")
    mine = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert mine == s["ccdm"] and mine == s["ldm"]
    assert (m.bert_max_length, m.bert_encode_batch, m.use_text_split, m.max_length) == (512, 1, False, 512)
    assert not m.transformer.training and not any(p.requires_grad for p in m.parameters())
    assert cond.FrozenBERTEmbedder(tiny, device="cpu", max_length=1024).bert_encode_batch == 2
    sd = bert_ref.seeded_state_dict(tiny_cfg(), "bert_tiny.")
    assert all(torch.equal(v, sd[k[len("transformer."):]]) for k, v in m.state_dict().items())
    ld = bert_ldm(tiny)
    assert [e for e in ([k, list(v.shape)] for k, v in ld.state_dict().items()) if e[0].startswith("cond_stage_model.")] == s["chain_cond_stage"]


def test_dotted_paths_resolve():
    from jointimagegeneration_amd import cond, encoder
    from jointimagegeneration_amd.config import get_obj_from_str
    assert get_obj_from_str("ldm.modules.encoders.modules.FrozenBERTEmbedder") is cond.FrozenBERTEmbedder
    assert get_obj_from_str("ddpm.models.encoder.FrozenBERTEmbedder") is cond.FrozenBERTEmbedder
    assert encoder.FrozenBERTEmbedder is cond.FrozenBERTEmbedder


def test_package_does_not_import_transformers():
    code = ("import sys; import jointimagegeneration_amd.cond, jointimagegeneration_amd.encoder, jointimagegeneration_amd.io, "
            "jointimagegeneration_amd.tokenizer; bad = [m for m in ('transformers', 'tokenizers', 'safetensors') if m in sys.modules]; "
            "assert not bad, bad")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


# ------------------------------------------------------------------------------------------------ tokenizer
def test_tokenizer_ids_and_masks_equal_the_reference(tiny):
    from jointimagegeneration_amd import cond
    s, g = surf(), gold("bert")
    m = cond.FrozenBERTEmbedder(tiny, device="cpu")
    assert len(s["strings"]) == 5 and s["strings"][0] == "" and len(s["strings"][2].split()[0]) == 101
    for i, text in enumerate(s["strings"]):
        ids, mask = m.tokenizer.encode([text], s["n_tok"])
        assert ids[0] == g["ids"][i].tolist(), (text, ids[0], g["ids"][i].tolist())
        assert mask[0] == g["mask"][i].tolist()
    ids, mask = m.tokenizer.encode(s["strings"], s["n_tok"])
    assert np.array_equal(np.array(ids), g["ids"]) and np.array_equal(np.array(mask), g["mask"])
    # what the strings exercise, stated on the ids: [CLS] [SEP] alone; an over-long word is [UNK]; truncation keeps [SEP]
    tk = m.tokenizer
    assert ids[0][:3] == [tk.cls, tk.sep, tk.pad] and ids[2][1] == tk.unk and ids[3][-1] == tk.sep and sum(mask[3]) == s["n_tok"]


def test_tokenizer_rules():
    from jointimagegeneration_amd.tokenizer import BertWordPieceTokenizer
    with open(os.path.join(TINY_DIR, "vocab.txt"), encoding="utf-8") as f:
        vocab = [line.rstrip("\n") for line in f]
    tk = BertWordPieceTokenizer(vocab, do_lower_case=True)
    v = tk.vocab
    assert tk.tokenize_ids("LIVER") == [v["liver"]] and tk.tokenize_ids("Café") == [v["cafe"]]
    assert tk.tokenize_ids("肝脏liver") == [v["肝"], v["脏"], v["liver"]]                     # CJK characters are isolated
    assert tk.tokenize_ids("segmentation") == [v["seg"], v["##ment"], v["##ation"]]
    assert tk.tokenize_ids("liverzz") == [tk.unk]                                          # a stretch no piece covers: the whole word
    assert tk.tokenize_ids("a[MASK]a [mask]") == [v["a"], v["[MASK]"], v["a"], v["["], tk.unk, v["]"]]      # never split; case matters
    assert tk.tokenize_ids("x" * 100) == [v["x"]] + [v["##x"]] * 99 and tk.tokenize_ids("x" * 101) == [tk.unk]
    assert tk.tokenize_ids("no\x00 \ufffdlesion\u200b\x07.") == [v["no"], v["lesion"], v["."]]                  # dropped characters
    cased = BertWordPieceTokenizer(vocab, do_lower_case=False)
    assert cased.tokenize_ids("Liver liver") == [tk.unk, v["liver"]]
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        BertWordPieceTokenizer(["[PAD]", "[UNK]", "[SEP]"])


# ------------------------------------------------------------------------------------------------ readers
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_safetensors_round_trip(tmp_path, dtype):
    from jointimagegeneration_amd import io as gio
    gen = torch.Generator().manual_seed(3)
    sd = {"a.weight": torch.randn(5, 7, generator=gen).to(dtype), "b": torch.randn(3, generator=gen).to(dtype),
          "c": torch.randn(2, 1, 4, generator=gen)}
    p = str(tmp_path / "m.safetensors")
    bert_ref.write_safetensors(p, sd)
    got = gio.read_safetensors(p)
    assert list(got) == list(sd)
    for k in sd:
        assert got[k].dtype == sd[k].dtype and got[k].shape == sd[k].shape and torch.equal(got[k], sd[k])


def test_safetensors_refusals(tmp_path):
    import struct
    from jointimagegeneration_amd import io as gio

    def write(header, payload=b"\0" * 16):
        hj = json.dumps(header).encode()
        p = str(tmp_path / "bad.safetensors")
        with open(p, "wb") as f:
            f.write(struct.pack("<Q", len(hj)) + hj + payload)
        return p

    with pytest.raises(NotImplementedError, match="I64"):
        gio.read_safetensors(write({"t": {"dtype": "I64", "shape": [2], "data_offsets": [0, 16]}}))
    with pytest.raises(ValueError, match="byte range"):
        gio.read_safetensors(write({"t": {"dtype": "F32", "shape": [8], "data_offsets": [0, 32]}}))
    with pytest.raises(ValueError, match="byte range"):
        gio.read_safetensors(write({"t": {"dtype": "F32", "shape": [3], "data_offsets": [0, 16]}}))
    p = str(tmp_path / "short.safetensors")
    with open(p, "wb") as f:
        f.write(struct.pack("<Q", 1 << 40) + b"{}")
    with pytest.raises(ValueError, match="header length"):
        gio.read_safetensors(p)


def test_bin_and_safetensors_give_equal_tensors(tmp_path, tiny):
    from jointimagegeneration_amd import cond
    a = cond.FrozenBERTEmbedder(tiny, device="cpu").state_dict()
    b = cond.FrozenBERTEmbedder(make_dir(tmp_path / "bin", fmt="bin"), device="cpu").state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(FileNotFoundError, match="pytorch_model.bin"):
        d = make_dir(tmp_path / "none", fmt="bin")
        os.remove(os.path.join(d, "pytorch_model.bin"))
        cond.FrozenBERTEmbedder(d, device="cpu")


def test_old_checkpoint_layouts_load(tmp_path):
    """embeddings.position_ids / token_type_ids buffers are ignored; the bert. prefix, the cls.* heads and LayerNorm.gamma / beta of old
    task-head checkpoints are mapped; under the embedder the prefix is transformer., so an LDM checkpoint's cond_stage_model keys load."""
    from jointimagegeneration_amd import cond
    cfg = tiny_cfg()
    sd = bert_ref.seeded_state_dict(cfg, "bert_tiny.")
    old = dict(sd)
    old["embeddings.position_ids"] = torch.arange(40)[None]
    old["embeddings.token_type_ids"] = torch.zeros(1, 40, dtype=torch.long)
    m = cond.FrozenBERTEmbedder(make_dir(tmp_path / "ids", fmt="bin", sd=old), device="cpu")
    assert all(torch.equal(v, sd[k[len("transformer."):]]) for k, v in m.state_dict().items())
    mlm = {"bert." + k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta"): v for k, v in old.items()}
    mlm["cls.predictions.bias"] = torch.zeros(128)
    m2 = cond.FrozenBERTEmbedder(make_dir(tmp_path / "mlm", fmt="bin", sd=mlm), device="cpu")
    assert all(torch.equal(v, sd[k[len("transformer."):]]) for k, v in m2.state_dict().items())
    ckpt = {"cond_stage_model.transformer." + k: v + 1 for k, v in old.items()}
    ld = bert_ldm(make_dir(tmp_path / "ld"))
    missing, unexpected = ld.load_state_dict(ckpt, strict=False)
    assert not unexpected and not any(k.startswith("cond_stage_model.") for k in missing)
    assert torch.equal(ld.cond_stage_model.transformer.pooler.dense.bias, sd["pooler.dense.bias"] + 1)
    with pytest.raises(RuntimeError, match="Missing key"):
        bad = dict(sd)
        del bad["pooler.dense.weight"]
        cond.FrozenBERTEmbedder(make_dir(tmp_path / "bad", sd=bad), device="cpu")


# ------------------------------------------------------------------------------------------------ text splitting, interleave
def test_merge_text_list_and_interleave_against_the_recorded_lists(tiny):
    from jointimagegeneration_amd import cond
    s, g = surf(), gold("bert")
    m = cond.FrozenBERTEmbedder(tiny, device="cpu")
    texts = [s["strings"][i] for i in s["split"]]
    m.use_text_split = True
    assert m._merge_text_list(*texts) == texts                                   # x = 1: unchanged
    m.bert_encode_batch = 2
    assert m._merge_text_list(*texts) == s["merged_x2"] == [texts[0], "", texts[1], ""]
    assert m._merge_text_list(7, ["a", "b", "c"]) == ["7", "", "a", "b"]         # str() of a non-list, a list cut to x, as the reference
    # the interleave, on the reference's own output: chunk xi of sample b on rows xi::x; the "" chunk is the same for every sample
    z2, x1 = torch.from_numpy(g["ccdm_x2"]), torch.from_numpy(g["ccdm_x1"])
    assert torch.equal(z2[0, 1::2], z2[1, 1::2])
    assert torch.allclose(z2[0, 0::2], x1[s["batch3"].index(s["split"][0])], atol=1e-5)
    assert torch.allclose(z2[0, 1::2], x1[s["batch3"].index(0)], atol=1e-5)     # STRINGS[0] is ""
    chunks = torch.stack([z2[0, 0::2], z2[0, 1::2], z2[1, 0::2], z2[1, 1::2]])
    assert torch.equal(bert_ref.interleave(chunks, 2), z2)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("over, match", [
    (dict(position_embedding_type="relative_key"), "position_embedding_type"),
    (dict(hidden_act="gelu_new"), "hidden_act"),
    (dict(is_decoder=True), "is_decoder"),
    (dict(add_cross_attention=True), "add_cross_attention"),
    (dict(num_attention_heads=4), "head dim"),                     # 64 / 4 = 16: no kernel instance
    (dict(hidden_size=60, num_attention_heads=7), "head dim"),
])
def test_config_refusals(over, match):
    from jointimagegeneration_amd import cond
    with pytest.raises(NotImplementedError, match=match):
        cond.BertModel(tiny_cfg(**over))


def test_embedder_refusals(tiny, tmp_path):
    from jointimagegeneration_amd import cond
    with pytest.raises(ValueError, match="max_length"):
        cond.FrozenBERTEmbedder(tiny, device="cpu", max_length=256)
    with pytest.raises(ValueError, match="multiple"):
        cond.FrozenBERTEmbedder(tiny, device="cpu", max_length=768)
    with pytest.raises(FileNotFoundError, match="not a directory"):
        cond.FrozenBERTEmbedder(str(tmp_path / "nowhere"), device="cpu")
    m = cond.FrozenBERTEmbedder(tiny, device="cpu")
    m.bert_max_length = 16
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # a CPU model
        m.encode(["liver"])
    with pytest.raises(RuntimeError, match="training mode"):
        m.train().encode(["liver"])
    m.eval()
    from jointimagegeneration_amd import ops
    with ops.fp32_validation(), pytest.raises(NotImplementedError, match="fp32_validation"):
        m.encode(["liver"])
    assert not ops.FP32
    m.use_text_split, m.bert_encode_batch = True, 3
    with pytest.raises(NotImplementedError, match="bert_encode_batch = 3 > 2"):
        m._merge_text_list("liver")
    m.bert_encode_batch = 2
    with pytest.raises(NotImplementedError, match="512 characters"):
        m._merge_text_list("y" * 512)
    assert m._merge_text_list("y" * 511) == ["y" * 511, ""]
    with pytest.raises(ValueError, match="max_position_embeddings 40"):        # T above the position table: before any launch
        m.transformer.run(torch.zeros(1, 41, dtype=torch.int32), [41])
    with pytest.raises(ValueError, match="key lengths"):
        m.transformer.run(torch.zeros(2, 8, dtype=torch.int32), [8, 0])


def test_mask_refusals():
    from jointimagegeneration_amd.cond import prefix_lengths
    assert prefix_lengths(torch.tensor([[1, 1, 0], [1, 1, 1], [1, 0, 0]])) == [2, 3, 1]
    with pytest.raises(NotImplementedError, match="row 1 is not a prefix"):
        prefix_lengths(torch.tensor([[1, 1, 0], [1, 0, 1]]))
    with pytest.raises(NotImplementedError, match="not a prefix"):
        prefix_lengths(torch.tensor([[0, 1, 1]]))
    with pytest.raises(ValueError, match="row 1 has length 0"):
        prefix_lengths(torch.tensor([[1, 0], [0, 0]]))
    with pytest.raises(ValueError, match="0/1"):
        prefix_lengths(torch.tensor([[2, 0]]))


def test_kvlen_host_refusals():
    """the descriptor checks of gg_attention_forward_kvlen that need no device: head dims without a key-length instance, null kv_len"""
    import ctypes as C
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    d = _lib.AttentionDesc()
    d.N, d.heads, d.Tq, d.Tkv = 1, 1, 8, 8
    d.ldq = d.ldk = d.ldv = d.ldo = 256
    d.hsq = d.hsk = d.hsv = d.hso = 256
    d.q = d.k = d.v = d.out = 64                      # never dereferenced: every call below is refused before a launch
    d.scale = 1.0
    for hd in (256, 384, 512, 48):
        d.head_dim = hd
        assert lib.gg_attention_forward_kvlen(C.byref(d), 64, None) == -3 and b"head_dim" in lib.gg_last_error()       # GG_ERR_UNSUPPORTED
    d.head_dim = 64
    assert lib.gg_attention_forward_kvlen(C.byref(d), None, None) == -1 and b"kv_len" in lib.gg_last_error()
    assert lib.gg_attention_forward_kvlen_f32(C.byref(d), None, None) == -1
    d.head_dim = 128
    assert lib.gg_attention_forward_kvlen_f32(C.byref(d), 64, None) == -3


def test_cli_help():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "jointimagegeneration_amd.cond", "--help"], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0 and "--bert" in r.stdout and "--text-file" in r.stdout and "--out" in r.stdout


# ------------------------------------------------------------------------------------------------ the key-length inputs have teeth
def test_varlen_inputs_catch_a_kernel_that_ignores_or_misreads_the_length():
    """attn_exact's fp32 emulation of the kernel on the attn_varlen buffers: walking exactly L keys gives the closed form; walking all
    Tkv_max rows (the length ignored), one key too many or one too few does not, in every regime that has a poison row to see."""
    import attn_exact as X
    import attn_varlen as V
    import shadow
    case = V.CASES[0]
    cpu = torch.device("cpu")
    for regime in X.REGIMES:
        p = V.build(case, regime, cpu)
        H, D, Tq, Tm = case.heads, case.D, case.Tq, case.Tkv_max
        qv = shadow.attention_view(p.q, case.N, Tq, H, D, *p.ld_hs_q, 0)
        kv = shadow.attention_view(p.kv, case.N, Tm, H, D, *p.ld_hs_kv, 0)
        vv = shadow.attention_view(p.kv, case.N, Tm, H, D, *p.ld_hs_kv, p.v_off)
        plan = (64, 1, 0, 0)
        for n, L in enumerate(case.lengths):
            emu = lambda keys: X.emulate_head(qv[n, :, 0], kv[n, :keys, 0], vv[n, :keys, 0], p.scale, plan)
            assert not X.mismatches(emu(L), p.want[n, :, 0]), (regime, L)
            if L < Tm:
                assert X.mismatches(emu(Tm), p.want[n, :, 0]), (regime, L, "length ignored")
                assert X.mismatches(emu(L + 1), p.want[n, :, 0]), (regime, L, "one key too many")
            if L > 1 and regime != "uni" or L > 2:
                assert X.mismatches(emu(L - 1), p.want[n, :, 0]), (regime, L, "one key too few")

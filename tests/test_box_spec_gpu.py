"""Shape-specialised box convs (gg_conv_box_spec.hip) against the generic box kernel, on the C5 latent UNet at batch 1.

Every conv of one N = 1 @64x64 forward with the fused DDIM head runs twice on the same device inputs: with path_hint GG_BOX_HINT_GENERIC
(the generic kernel) and with GG_BOX_HINT_SPEC_ONLY (a box conv without a table entry is an error).  Outputs, the GroupNorm fixed-point
sums each conv leaves in the accumulator arena and the DDIM state must be byte for byte the same; the table must hold exactly the
configurations the network reaches."""
import importlib.util
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINT_GENERIC, HINT_SPEC_ONLY = 10, 11          # GG_BOX_HINT_GENERIC / GG_BOX_HINT_SPEC_ONLY (gg_conv.h)

pytestmark = pytest.mark.gpu


def _gen():
    spec = importlib.util.spec_from_file_location("gen_box_specs", os.path.join(ROOT, "tools", "gen_box_specs.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _c5_unet(dev):
    from jointimagegeneration_amd.synth import randomize_parameters
    from jointimagegeneration_amd.unet import UNetModel
    u = UNetModel(dims=2, image_size=512, in_channels=8, out_channels=4, model_channels=160, attention_resolutions=[8, 4, 2],
                  num_res_blocks=2, channel_mult=[1, 2, 4, 4, 5], num_head_channels=32).eval()
    randomize_parameters(u, 1024, "ldm.")
    return u.to(dev)


def test_table_is_exactly_the_c5_batch1_box_convs():
    """No dead entries and no missing ones: the keys the library traces for the C5 forward (plan_box's plans) are the table."""
    g = _gen()
    table, traced = g.table_keys(), g.traced_keys()
    assert len(table) == len(set(table))
    assert set(table) == set(traced), (sorted(set(table) - set(traced)), sorted(set(traced) - set(table)))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_specialised_equals_generic_bytewise(monkeypatch):
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ops import CL
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    # every conv runs twice, and both runs leave their sums: room for two forwards' worth in the arena
    monkeypatch.setattr(ops, "_ARENA_ENTRIES", 1 << 21)
    monkeypatch.setattr(ops, "_ARENAS", {})
    torch.manual_seed(0)
    u = _c5_unet(dev)
    x = CL(torch.randn(1, 1, 64, 64, 32, device=dev).bfloat16(), 8)
    row = u.time_bias_rows(torch.full((1,), 981.0, device=dev))
    M = 64 * 64
    xs = torch.randn(M, 4, device=dev)
    scal = torch.tensor([0.5, 0.6, 0.0, 0.7], device=dev)
    px0 = torch.zeros(M, 4, device=dev)
    eps = torch.empty(1, 1, 64, 64, 32, device=dev)

    real = ops.conv
    seen = dict(calls=0, stats=0, ddim=0, flags=set())

    sig = inspect.signature(real)

    def spy(*args, **kwargs):
        ba = sig.bind(*args, **kwargs)
        ba.apply_defaults()
        kw = dict(ba.arguments)
        seen["calls"] += 1
        kg = dict(kw)
        if kw.get("out") is not None:
            kg["out"] = torch.empty_like(kw["out"])
        dd = kw.get("ddim")
        state = [t for t in ((dd[0], dd[2], dd[3]) if dd is not None else ()) if t is not None]
        before = [t.clone() for t in state]
        old = ops.PATH_HINT
        try:
            ops.PATH_HINT = HINT_GENERIC
            g = real(**kg)
            after_g = [t.clone() for t in state]
            for t, b in zip(state, before):
                t.copy_(b)
            ops.PATH_HINT = HINT_SPEC_ONLY
            s = real(**kw)
        finally:
            ops.PATH_HINT = old
        torch.cuda.synchronize()
        assert _same(g.t, s.t), f"conv #{seen['calls']}: outputs differ"
        assert (g.acc is None) == (s.acc is None) and g.fused_ddim == s.fused_ddim
        if s.acc is not None:
            seen["stats"] += 1
            assert _same(g.acc, s.acc), f"conv #{seen['calls']}: GroupNorm sums differ"
        if s.fused_ddim:
            seen["ddim"] += 1
            for a, b in zip(after_g, state):
                assert _same(a, b), f"conv #{seen['calls']}: DDIM state differs"
        seen["flags"].update(k for k in ("residual", "prologue", "prologue_acc", "skip", "src2") if kw.get(k) is not None)
        seen["flags"].update(k for k in ("upsample",) if kw.get(k))
        if kw["stride"] == 2:
            seen["flags"].add("stride2")
        return s

    monkeypatch.setattr(ops, "conv", spy)
    u.forward_cl(x, row)
    head = u.forward_cl(x, row, None, head_out=eps, head_ddim=(xs, scal, px0, x.t.view(M, -1)))
    assert head.fused_ddim
    assert seen["ddim"] == 1 and seen["stats"] > 0
    # every flag combination the table holds was exercised
    assert {"residual", "prologue_acc", "skip", "upsample", "stride2"} <= seen["flags"], seen["flags"]

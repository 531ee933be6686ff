"""CPU suite for latent inpainting (mask= / x0= of the DDIM, PLMS and ancestral samplers): operand validation, the q_sample scalar table,
the options that stay refused, and the host-side argument checks of gg_inpaint_blend (its declaration is checked with every other in test_capi_cpu.py)."""
import re

import numpy as np
import pytest
import torch

from util import small_ldm

SHAPE = (2, 4, 8, 8)


@pytest.fixture(scope="module")
def model():
    return small_ldm()


# ------------------------------------------------------------------------------------------------ operand validation
def test_mask_without_x0_is_refused():
    from jointimagegeneration_amd.ldm import inpaint_operands
    with pytest.raises(ValueError, match="without x0"):
        inpaint_operands(torch.ones(2, 1, 8, 8), None, SHAPE)
    assert inpaint_operands(None, torch.zeros(SHAPE), SHAPE) is None          # x0 alone is ignored, as in the reference
    assert inpaint_operands(None, None, SHAPE) is None


@pytest.mark.parametrize("x0_shape", [(2, 4, 8, 7), (3, 4, 8, 8), (2, 3, 8, 8), (2, 4, 8), (1, 2, 4, 8, 8), (2, 4, 16, 16)])
def test_x0_that_does_not_broadcast_is_refused(x0_shape):
    from jointimagegeneration_amd.ldm import inpaint_operands
    with pytest.raises(ValueError, match=re.escape(str(tuple(x0_shape)))):
        inpaint_operands(torch.ones(2, 1, 8, 8), torch.zeros(x0_shape), SHAPE)


@pytest.mark.parametrize("mask_shape", [(2, 2, 8, 8), (2, 1, 8, 4), (3, 1, 8, 8), (1, 2, 1, 8, 8), (2, 1, 16, 16), (2, 8)])
def test_mask_that_does_not_broadcast_is_refused(mask_shape):
    from jointimagegeneration_amd.ldm import inpaint_operands
    with pytest.raises(ValueError, match=re.escape(str(tuple(mask_shape)))):
        inpaint_operands(torch.ones(mask_shape), torch.zeros(SHAPE), SHAPE)


@pytest.mark.parametrize("mask_shape,cm", [((2, 1, 8, 8), 1), ((2, 4, 8, 8), 4), ((1, 1, 8, 8), 1), ((8, 8), 1), ((1, 8), 1),
                                           ((4, 1, 1), 4), ((1, 4, 8, 8), 4), ((), 1)])
def test_accepted_broadcasts_and_channel_extent(mask_shape, cm):
    from jointimagegeneration_amd.ldm import inpaint_operands
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(mask_shape, generator=g)
    x0 = torch.randn(1, 4, 1, 8, generator=g)                      # x0 broadcasts too
    x0e, me, got_cm = inpaint_operands(mask, x0, SHAPE)
    assert got_cm == cm
    assert tuple(x0e.shape) == SHAPE and torch.equal(x0e, x0.expand(SHAPE))
    assert tuple(me.shape) == (2, cm, 8, 8) and me.dtype == torch.float32
    assert torch.equal(me.expand(SHAPE), mask.expand(SHAPE))       # the kept channel extent broadcasts back to the same values


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int32, torch.int64, torch.float16, torch.float64])
def test_non_fp32_masks_are_cast(dtype):
    from jointimagegeneration_amd.ldm import inpaint_operands
    hole = torch.ones(2, 1, 8, 8, dtype=torch.bool)
    hole[:, :, 2:6, 2:6] = False
    x0e, me, cm = inpaint_operands(hole.to(dtype), torch.zeros(SHAPE, dtype=torch.float64), SHAPE)
    assert me.dtype == torch.float32 and x0e.dtype == torch.float32 and cm == 1
    assert torch.equal(me, hole.float())


def test_mask_noise_tape_is_checked():
    from jointimagegeneration_amd.ldm import inpaint_operands
    m, x0 = torch.ones(2, 1, 8, 8), torch.zeros(SHAPE)
    assert inpaint_operands(m, x0, SHAPE, [torch.zeros(SHAPE)] * 5, 5) is not None
    with pytest.raises(ValueError, match="holds 4 tensors"):
        inpaint_operands(m, x0, SHAPE, [torch.zeros(SHAPE)] * 4, 5)
    with pytest.raises(ValueError, match=re.escape("mask_noise_tape[2]")):
        inpaint_operands(m, x0, SHAPE, [torch.zeros(SHAPE)] * 2 + [torch.zeros(2, 1, 8, 8)] * 3, 5)


def test_samplers_validate_before_any_launch(model):
    """The refusals below come from host code on CPU tensors: nothing reached the GPU (there is none here)."""
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    for cls in (DDIMSampler, PLMSSampler):
        with pytest.raises(ValueError, match="without x0"):
            cls(model).sample(S=5, batch_size=2, shape=(4, 8, 8), verbose=False, mask=torch.ones(2, 1, 8, 8))
        with pytest.raises(ValueError, match=re.escape("(2, 4, 4, 4)")):
            cls(model).sample(S=5, batch_size=2, shape=(4, 8, 8), verbose=False, mask=torch.ones(2, 1, 8, 8), x0=torch.zeros(2, 4, 4, 4))
    with pytest.raises(ValueError, match="without x0"):
        model.p_sample_loop(None, SHAPE, mask=torch.ones(2, 1, 8, 8))
    with pytest.raises(ValueError, match="differ in spatial size"):                     # ddpm.py:1200's assert
        model.p_sample_loop(None, SHAPE, mask=torch.ones(2, 1, 1, 8), x0=torch.zeros(SHAPE))
    with pytest.raises(ValueError, match="mask_noise_tape"):
        model.p_sample_loop(None, SHAPE, timesteps=3, mask=torch.ones(2, 1, 8, 8), x0=torch.zeros(SHAPE), mask_noise_tape=[torch.zeros(SHAPE)])


# ------------------------------------------------------------------------------------------------ scalar table
@pytest.mark.parametrize("steps,discretize", [(5, "uniform"), (50, "uniform"), (6, "quad")])
def test_q_sample_scalar_table_reads_the_model_buffers_in_sampling_order(model, steps, discretize):
    from jointimagegeneration_amd.ldm import DDIMSampler
    s = DDIMSampler(model)
    s.make_schedule(steps, ddim_discretize=discretize, verbose=False)
    tab = s.q_sample_scalar_table()
    ts = np.flip(s.ddim_timesteps)
    assert tab.shape == (steps, 2) and tab.dtype == torch.float32
    assert ts[0] == s.ddim_timesteps.max() and ts[-1] == s.ddim_timesteps.min() >= 1          # 1-based DDPM steps, latest first
    for i, t in enumerate(ts):
        assert tab[i, 0].item() == model.sqrt_alphas_cumprod[int(t)].item()
        assert tab[i, 1].item() == model.sqrt_one_minus_alphas_cumprod[int(t)].item()
    # the buffers, not values recomputed from ddim_alphas (those differ in the last bits at some steps)
    recomputed = torch.sqrt(s.ddim_alphas.flip(0))
    assert torch.allclose(tab[:, 0], recomputed, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ still refused
@pytest.mark.parametrize("kw,name", [(dict(quantize_x0=True), "quantize_x0"), (dict(score_corrector=object()), "score_corrector"),
                                     (dict(noise_dropout=0.1), "noise_dropout"), (dict(temperature=0.5), "temperature")])
def test_still_refused_options_name_themselves(model, kw, name):
    from jointimagegeneration_amd.ldm import DDIMSampler
    with pytest.raises(NotImplementedError) as ei:
        DDIMSampler(model).sample(S=5, batch_size=2, shape=(4, 8, 8), verbose=False, **kw)
    assert name in str(ei.value) and "inpaint" not in str(ei.value)
    with pytest.raises(NotImplementedError, match="quantize_denoised") as ei:
        model.p_sample_loop(None, SHAPE, quantize_denoised=True)
    assert "inpaint" not in str(ei.value)


def test_encode_first_stage_refuses_split_input_params(model):
    model.split_input_params = dict(patch_distributed_vq=True)
    try:
        with pytest.raises(NotImplementedError, match="split_input_params"):
            model.encode_first_stage(torch.zeros(1, 1, 32, 32))
    finally:
        del model.split_input_params


def test_get_first_stage_encoding_scales(model):
    from jointimagegeneration_amd.ldm import DiagonalGaussianDistribution
    x = torch.randn(2, 4, 8, 8)
    model.scale_factor = 0.5
    try:
        assert torch.equal(model.get_first_stage_encoding(x), 0.5 * x)
        post = DiagonalGaussianDistribution(torch.cat([x, torch.full_like(x, -30.0)], 1))        # std = exp(-15): sample ~ mean
        assert torch.allclose(model.get_first_stage_encoding(post), 0.5 * x, atol=1e-5)
        with pytest.raises(NotImplementedError):
            model.get_first_stage_encoding([x])
    finally:
        model.scale_factor = 1.0


# ------------------------------------------------------------------------------------------------ C-ABI
def test_gg_inpaint_blend_rejects_bad_arguments_on_the_host():
    """Every check runs before a launch, so the error codes are observable without a GPU (the fake pointers are never read)."""
    from util import load_lib
    lib = load_lib()
    p = 0x1000
    bad_shape = -1
    assert lib.gg_inpaint_blend(p, p, p, 3, p, p, 16, 4, None, 0, None) == bad_shape          # mask_C neither 1 nor C
    assert b"mask_C" in lib.gg_last_error()
    assert lib.gg_inpaint_blend(p, p, p, 2, p, p, 16, 4, None, 0, None) == bad_shape
    assert lib.gg_inpaint_blend(p, p, p, 1, p, p, 16, 4, p, 3, None) == bad_shape             # unet_in_stride < C
    for i in (0, 1, 2, 4, 5):                                                                  # null x, x0, mask, noise, scalars
        a = [p, p, p, 1, p, p]
        a[i] = None
        assert lib.gg_inpaint_blend(*a, 16, 4, None, 0, None) == bad_shape, i
    assert lib.gg_inpaint_blend(p, p, p, 1, p, p, 0, 4, p, 32, None) == 0                      # M = 0: nothing to do, no launch
    assert lib.gg_inpaint_blend(p, p, p, 3, p, p, 0, 3, None, 0, None) == 0

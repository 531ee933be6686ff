"""Stale-state harness: does every cache and captured graph follow the inputs it was built from?

Between the kernels and a caller sits host state that outlives a launch: repacked weights, per-schedule tables, static buffers, captured
hipGraphs.  A stale entry raises nothing; it returns a plausible result computed from old weights or an old schedule, and no kernel test
can see that, because every kernel did what it was told.  `check_follows` runs one long-lived object (a sampler, a pipeline, a loss
module) before and after a mutation of something its caches were built from, and compares what it returns after the mutation, bit for
bit, with what freshly built objects return on the mutated model.  The two sides run the same kernels on the same inputs in the same
order, the project demands graph == eager bit for bit and its GroupNorm sums are integer atomics, so `torch.equal` is the bound.

INVENTORY is the table of those caches; tests/test_stale_state_cpu.py holds it against the package's source, so that a cache added later
fails there until it has a row and a case in tests/test_stale_state_gpu.py."""
import contextlib
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "jointimagegeneration_amd")
GPU_TESTS = os.path.join(ROOT, "tests", "test_stale_state_gpu.py")
CALLS = 3                                   # the ladder of ops.replay_captured: eager, capture + replay, replay
SITES = ("weights_token(", "PACKED.get(", "capture_graph(", "replay_captured(")


# ------------------------------------------------------------------------------------------------ the inventory
def row(cache, holder, file, sites, key, token, bakes, cases):
    return dict(cache=cache, holder=holder, file=file, sites=dict(sites), key=key, token=token, bakes=dict(bakes), cases=sorted({c for v in bakes.values() for c in v} | set(cases)))


# One row per cache.  sites: how many call sites of each SITES pattern in `file` belong to the row (definitions, `def name(`, are not call
# sites).  bakes: what the cached value was computed from -> the GPU tests that change exactly that and require the result to follow.
INVENTORY = [
    row("packed conv / linear weights and padded biases", "blocks.PACKED", "blocks.py", {"PACKED.get(": 5},
        "(id(module), cin_pad, tag, ops.FP32)", "(data_ptr, _version) of the parameters + weak references to them",
        {"the parameters' values": ["test_ldm_chain_follows_a_weight_written_in_place", "test_ldm_chain_follows_load_state_dict",
                                    "test_pipeline_follows_a_stage_weight", "test_ccdm_labels_follow_a_unet_weight"],
         "values written through .data (after ops.invalidate_caches)": ["test_ldm_chain_follows_a_data_write_after_invalidate_caches"],
         "ops.FP32": ["test_loss_modules_follow_fp32_validation_entered_and_left"],
         "a freed module's id and storage reused": []}, ["test_harness_reports_a_planted_stale_token"]),
    row("chain state (chain.new_state): time-bias table, step scalars, q_sample scalars, static buffers, chain graph", "DDIMSampler._graphs (PLMS, DPM-Solver alike)",
        "ldm.py", {"weights_token(": 1, "replay_captured(": 1},
        "(N, Cx, sp3, Cc, device, ctx_shape) + state_tag + inpaint / vq / log / split entries",
        "(S, ddim_timesteps, ddim_sigmas, weights_token(unet), step / q_sample scalar tables) + the codebook's identity",
        {"UNet weights": ["test_ldm_chain_follows_a_weight_written_in_place", "test_ldm_chain_follows_load_state_dict",
                          "test_ldm_chain_follows_a_data_write_after_invalidate_caches", "test_dpm_solver_chain_follows"],
         "alphas_cumprod at the chain's timesteps (scal)": ["test_ldm_chain_follows_the_schedule", "test_dpm_solver_chain_follows"],
         "sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod (ip_scal)": ["test_inpainting_state_follows_the_schedule"],
         "timesteps (discretisation) and sigmas (eta)": ["test_ldm_chain_follows_discretisation_and_eta"],
         "the VQ codebook": ["test_vq_state_follows_the_codebook"],
         "temperature (fifth scalar column; no rebuild)": ["test_same_shape_inputs_reuse_state_and_graph"],
         "context, x_T, guidance scale (static buffers; no rebuild)": ["test_same_shape_inputs_reuse_state_and_graph"],
         "split_input_params": ["test_split_state_follows_its_geometry"],
         "log_every_t": ["test_logged_state_follows_log_every_t"],
         "fuse_ddim, use_graph (read at capture)": ["test_ldm_chain_follows_fuse_ddim_and_use_graph"],
         "DPM-Solver order / clip_denoised (state_tag)": ["test_dpm_solver_chain_follows"]}, ["test_harness_reports_a_planted_stale_token"]),
    row("slice / volume engines: static buffers, encode / decode heads, per-slice graph", "GuideGenPipeline._slice_graphs / _volume_graphs",
        "pipeline.py", {"weights_token(": 2, "capture_graph(": 2, "replay_captured(": 2},
        "(N, hw, device) / (B, hw, depth, label shape, device) + edit entry",
        "(id(chain state), weights_token(cond_stage_model), weights_token(first_stage_model), scale_factor)",
        {"cond_stage_model weights": ["test_pipeline_follows_a_stage_weight"],
         "first_stage_model weights": ["test_pipeline_follows_a_stage_weight"],
         "ldm.scale_factor (float, or the scale_by_std buffer)": ["test_pipeline_follows_scale_factor"],
         "the chain state (schedule of ldm)": ["test_pipeline_follows_the_schedule"]}, []),
    row("CCDM step graph (lives for one sample_labels call)", "LabelChain.ladder, the state DenoisingModel.sample_labels builds per call", "ccdm.py",
        {"replay_captured(": 1}, "none: rebuilt per call", "none",
        {"UNet weights": ["test_ccdm_labels_follow_a_unet_weight"], "the diffusion schedule": ["test_ccdm_labels_follow_the_schedule"]}, []),
    row("LPIPS packs", "LPIPS._packs", "lpips.py", {"weights_token(": 1}, "ops.FP32", "(ops.FP32, weights_token(self), identity of shift / scale)",
        {"conv weights": ["test_loss_modules_follow_a_conv_weight"], "shift / scale buffers": ["test_lpips_follows_shift_and_scale"],
         "ops.FP32": ["test_loss_modules_follow_fp32_validation_entered_and_left"]}, []),
    row("PatchGAN packs (BatchNorm folded in fp64) and the VGG-loaded check", "NLayerDiscriminator._packs / LPIPSWithDiscriminator._vgg_checked",
        "aeloss.py", {"weights_token(": 1}, "ops.FP32", "(ops.FP32, parameters and buffers: count, versions, addresses)",
        {"conv weights": ["test_loss_modules_follow_a_conv_weight"], "BatchNorm running statistics": ["test_discriminator_follows_a_running_statistic"],
         "ops.FP32": ["test_loss_modules_follow_fp32_validation_entered_and_left"]}, []),
    row("the graph ladder itself", "ops.replay_captured", "ops.py", {"capture_graph(": 1}, "holder[slot]", "holder['warmed']",
        {"the launch sequence of `body`": ["test_ldm_chain_follows_fuse_ddim_and_use_graph"]}, []),
    row("GroupNorm statistics arena", "ops._ARENAS", "ops.py", {}, "str(device)", "none: bump-allocated per forward, zeroed at its start",
        {"_ARENA_ENTRIES (a full arena answers None)": ["test_arena_of_zero_entries_equals_gn_acc_off", "test_arena_filling_mid_forward_stays_in_bounds_and_leaves_nothing"]},
        []),
]


def scan_sites():
    """{(file, pattern): count} of the call sites of SITES in the package's Python files (`def name(` is a definition, not a site)."""
    out = {}
    for name in sorted(os.listdir(PACKAGE)):
        if not name.endswith(".py"):
            continue
        with open(os.path.join(PACKAGE, name)) as f:
            text = f.read()
        for pat in SITES:
            n = len(re.findall(r"(?<!def )" + re.escape(pat), text))
            if n:
                out[(name, pat)] = n
    return out


def table_sites():
    out = {}
    for r in INVENTORY:
        for pat, n in r["sites"].items():
            out[(r["file"], pat)] = out.get((r["file"], pat), 0) + n
    return out


def gpu_test_names():
    with open(GPU_TESTS) as f:
        return set(re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))


# ------------------------------------------------------------------------------------------------ the harness
def same(a, b) -> bool:
    """Bit equality of two results: tensors, or equally long sequences of results."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


def snapshot(r):
    return r.clone() if isinstance(r, torch.Tensor) else tuple(snapshot(x) for x in r)


@contextlib.contextmanager
def fresh_packed():
    """blocks.PACKED replaced by an empty cache for the duration of the block."""
    import pytest
    from jointimagegeneration_amd import blocks
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(blocks, "PACKED", blocks._Packed())
        yield


def follow(make_objects, run, mutate, held=None):
    """The runs of `check_follows` without its verdict: a list with one entry per mutation, dict(got=[CALLS results of the long-lived
    object after the mutation], want=[CALLS results of fresh objects on the mutated model], before=the last result before it)."""
    model, obj = make_objects(None)
    for _ in range(CALLS):
        before = snapshot(run(model, obj))
    if held is not None:
        slots = list(held(obj))
        assert slots and all(s is not None for s in slots), f"no captured graph is held, the case would only run eager code: {slots}"
    stages = []
    for m in (mutate if isinstance(mutate, (list, tuple)) else [mutate]):
        m(model, obj)
        got = [snapshot(run(model, obj)) for _ in range(CALLS)]
        with fresh_packed():
            _, fresh = make_objects(model)
            want = [snapshot(run(model, fresh)) for _ in range(CALLS)]
            del fresh
        stages.append(dict(got=got, want=want, before=before, moves=getattr(m, "moves", True)))
        before = want[-1]
    return stages


def verdict(stages):
    """Per mutation: (follows at each call, the mutation moved the result, it was meant to)."""
    return [([same(g, w) for g, w in zip(s["got"], s["want"])], not same(s["before"], s["want"][-1]), s["moves"]) for s in stages]


def check_follows(make_objects, run, mutate, held=None):
    """make_objects(model or None) -> (model, obj): builds the model where none is given, and the long-lived object on it.
    run(model, obj) -> a tensor or a tuple of tensors, from fixed inputs.  mutate(model, obj), or a list of such, applied one after the
    other.  held(obj) -> the graph slots that must be filled after the first CALLS runs.
    After each mutation the object's CALLS results must equal, bit for bit, those of fresh objects built on the mutated model with an
    empty blocks.PACKED; and the mutation must have moved the result (what fresh objects return, against what they returned before
    it), else the case proves nothing.  A mutation with the attribute `moves = False` is a switch between two paths that the project
    requires to agree bit for bit: it must not move the result."""
    for i, (follows, moved, moves) in enumerate(verdict(follow(make_objects, run, mutate, held))):
        assert moved or not moves, f"mutation {i} did not move the result: the case proves nothing"
        assert moves or not moved, f"mutation {i} moved the result, and must not"
        assert all(follows), f"after mutation {i} the long-lived object does not return what fresh objects return (per call: {follows})"


class Launches:
    """Counts calls through the named ops entry points while the block runs (the idiom of test_vq_gpu's default-call test)."""
    NAMES = ("conv", "ddim_step", "ddim_step_vq", "vq_nearest", "inpaint_blend", "lincomb4", "capture_graph", "pack_conv_weight", "to_cl")

    def __init__(self):
        self.n = {name: 0 for name in self.NAMES}

    def __enter__(self):
        import pytest
        from jointimagegeneration_amd import ops
        self.mp = pytest.MonkeyPatch()
        for name in self.NAMES:
            real = getattr(ops, name)
            self.mp.setattr(ops, name, (lambda real, name: lambda *a, **k: (self.n.__setitem__(name, self.n[name] + 1), real(*a, **k))[1])(real, name))
        return self

    def __exit__(self, *exc):
        self.mp.undo()
        return False


def launches(fn):
    with Launches() as c:
        out = fn()
    return out, c.n

"""Region-based MultiDiffusion, host side: known answers of the mask front end, the spread / masked-mean identity, every refusal of
StableDiffusionRegionPipeline (raised before any device work: the pipeline object here has no engine at all), generation.py's region
flags, and the new C-ABI symbols."""
import ctypes
import json
import os
import re
import types

import pytest
import torch

import _regions_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("agd_op_region_masks", "agd_op_region_spread", "agd_op_region_mean", "agd_denoise_regions")


# ---- the mask front end ---------------------------------------------------------------------------------------------------------
def test_box_known_answer():
    from agenda_amd.regions import rasterize_boxes
    px = rasterize_boxes([[0.25, 0.25, 0.75, 0.75]], 128, 128)
    assert px.shape == (1, 128, 128) and px.dtype == torch.uint8
    assert torch.equal(px, R.boxes_to_masks([[0.25, 0.25, 0.75, 0.75]], 128, 128))
    m = R.latent_masks(px, 1, 16, 16)
    assert m.shape == (2, 1, 16, 16)
    want = torch.zeros(16, 16)
    want[4:12, 4:12] = 1                                        # latent rows and columns 4 .. 11 of 16
    assert torch.equal(m[1, 0], want) and torch.equal(m[0, 0], 1 - want)


def test_nearest_sample_reads_pixel_8y_8x():
    y, x = 3, 5
    off = torch.zeros(1, 128, 128, dtype=torch.uint8)
    off[0, 8 * y + 1, 8 * x] = 255                              # not on the sampling grid
    assert float(R.latent_masks(off, 1, 16, 16)[1].sum()) == 0.0
    on = torch.zeros(1, 128, 128, dtype=torch.uint8)
    on[0, 8 * y, 8 * x] = 255
    m = R.latent_masks(on, 1, 16, 16)
    assert float(m[1].sum()) == 1.0 and float(m[1, 0, y, x]) == 1.0 and float(m[0, 0, y, x]) == 0.0
    # float input thresholds at 0.5, uint8 at 127
    f = torch.zeros(1, 128, 128)
    f[0, 8 * y, 8 * x], f[0, 0, 0] = 0.51, 0.5
    mf = R.latent_masks(f, 1, 16, 16)
    assert float(mf[1].sum()) == 1.0 and float(mf[1, 0, y, x]) == 1.0
    u = torch.zeros(1, 128, 128, dtype=torch.uint8)
    u[0, 8 * y, 8 * x], u[0, 0, 0] = 128, 127
    assert torch.equal(R.latent_masks(u, 1, 16, 16), mf)


def test_overlapping_boxes_background_is_zero_on_their_union():
    px = R.boxes_to_masks([[0.0, 0.0, 0.5, 0.5], [0.25, 0.25, 0.75, 0.75]], 128, 128)
    m = R.latent_masks(px, 2, 16, 16)
    union = ((m[1] + m[2]) > 0).float()
    assert float((m[1] * m[2]).sum()) > 0                       # they do overlap
    assert torch.equal(m[0], 1 - union)
    assert torch.equal(m[:, 0], m[:, 1])                        # shared masks: the images' rows are equal


def test_mean_of_spread_is_the_canvas_without_bootstrapping():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 16, 24, generator=g)
    px = R.boxes_to_masks([[0.0, 0.0, 0.5, 1.0], [0.25, 0.0, 1.0, 0.5]], 128, 192)
    m = R.latent_masks(px, 2, 16, 24)
    back = R.masked_mean(R.spread(x, m), m)
    assert torch.allclose(back, x, rtol=1e-6, atol=1e-6)
    # and with bootstrapping the covered elements of a foreground region are the canvas, the others the noised background
    bg, n = torch.randn(3, 4, 16, 24, generator=g), torch.randn(2, 4, 16, 24, generator=g)
    xr = R.spread(x, m, n, bg, [2, 0], 0.6, 0.8).reshape(3, 2, 4, 16, 24)
    assert torch.equal(xr[0], x)
    cov = m[1][:, None].expand(-1, 4, -1, -1) > 0
    assert torch.equal(xr[1][cov], x[cov])
    assert torch.allclose(xr[1][~cov], (0.6 * bg[2][None] + 0.8 * n)[~cov])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _stub(scheduler="DDIMScheduler", in_channels=4, hooker=None, deepcache=None, ip_adapter=None):
    """A pipeline object with no engine: any device work would raise AttributeError, not the refusal under test."""
    from agenda_amd import StableDiffusionRegionPipeline
    from agenda_amd import scheduler as S
    from agenda_amd.config import CONFIGS
    pipe = object.__new__(StableDiffusionRegionPipeline)
    cfg = CONFIGS["sd15"]()
    cfg.unet = types.SimpleNamespace(in_channels=in_channels, out_channels=4)
    pipe.cfg = cfg
    pipe.vae_scale_factor = 8
    pipe.scheduler = S.SCHEDULERS[scheduler].from_config(cfg.sched)
    pipe._hooker, pipe._trace, pipe._lora, pipe._deepcache, pipe._ip_adapter = hooker, None, None, deepcache, ip_adapter
    return pipe


EMB = dict(prompt_embeds=torch.zeros(2, 77, 768), region_prompt_embeds=torch.zeros(2, 2, 77, 768))
BOXES = [[0.0, 0.0, 0.5, 1.0], [0.5, 0.0, 1.0, 1.0]]


def _call(pipe=None, **kw):
    args = dict(EMB, region_boxes=BOXES)
    args.update(kw)
    return (pipe or _stub())(**args)


@pytest.mark.parametrize("name", ["PNDMScheduler", "DPMSolverMultistepScheduler"])
def test_refuses_multistep_schedulers_by_name(name):
    with pytest.raises(ValueError) as e:
        _call(_stub(name))
    assert name in str(e.value) and 'scheduler="DDIMScheduler"' in str(e.value)


def test_refuses_img2img():
    with pytest.raises(NotImplementedError, match="img2img with region prompts"):
        _stub().img2img("a prompt", image=torch.zeros(1, 3, 64, 64))


def test_refuses_an_installed_hooker():
    with pytest.raises(ValueError, match="UNetCrossAttentionHooker"):
        _call(_stub(hooker=object()))


def test_refuses_an_inpainting_unet():
    with pytest.raises(ValueError, match="9 input channels"):
        _call(_stub(in_channels=9))


@pytest.mark.parametrize("kw,what", [({"guidance_rescale": 0.7}, "guidance_rescale=0.7"), ({"pag_scale": 3.0}, "pag_scale=3.0"),
                                     ({"max_embeddings_multiples": 2}, "max_embeddings_multiples=2")])
def test_refuses_arguments_of_the_plain_pipeline(kw, what):
    with pytest.raises(ValueError) as e:
        _call(**kw)
    assert what in str(e.value) and "StableDiffusionRegionPipeline" in str(e.value)


def test_refuses_an_enabled_deepcache():
    with pytest.raises(ValueError, match=r"DeepCache \(cache_interval=3"):
        _call(_stub(deepcache=(3, 0)))
    with pytest.raises(AttributeError):                          # interval 1 sets nothing and is not refused
        _call(_stub(deepcache=(1, 0)))


def test_refuses_a_long_context():
    with pytest.raises(ValueError, match="152 tokens"):
        _call(prompt_embeds=torch.zeros(2, 152, 768))
    with pytest.raises(ValueError, match="152 tokens"):
        _call(region_prompt_embeds=torch.zeros(2, 2, 152, 768))


def test_refuses_an_active_ip_adapter():
    with pytest.raises(ValueError, match="IP-Adapter"):
        _call(_stub(ip_adapter={"scale": 0.5}))
    with pytest.raises(ValueError, match="IP-Adapter"):
        _call(ip_adapter_image_embeds=torch.zeros(1, 1024))
    with pytest.raises(AttributeError):                          # an idle adapter (scale 0) is allowed
        _call(_stub(ip_adapter={"scale": 0.0}))


def test_refuses_both_or_neither_of_masks_and_boxes():
    masks = torch.zeros(2, 512, 512, dtype=torch.uint8)
    with pytest.raises(ValueError, match="exactly one of region_masks and region_boxes.*both"):
        _call(region_masks=masks)
    with pytest.raises(ValueError, match="exactly one of region_masks and region_boxes.*neither"):
        _call(region_boxes=None)


def test_refuses_wrong_counts_and_sizes():
    with pytest.raises(ValueError, match="1 region boxes for 2 region prompts"):
        _call(region_boxes=BOXES[:1])
    with pytest.raises(ValueError, match="3 region masks for 2 region prompts"):
        _call(region_boxes=None, region_masks=torch.zeros(3, 512, 512))
    with pytest.raises(ValueError, match="region_masks are 256 x 512, the image is 512 x 512"):
        _call(region_boxes=None, region_masks=torch.zeros(2, 256, 512))
    with pytest.raises(ValueError, match="per-image region masks for 3 images, the call makes 1"):
        _call(region_boxes=None, region_masks=torch.zeros(3, 2, 512, 512))
    with pytest.raises(ValueError, match="at most 8 regions"):
        _call(region_prompt_embeds=torch.zeros(8, 2, 77, 768), region_boxes=[BOXES[0]] * 8)


@pytest.mark.parametrize("box", [[0.5, 0.0, 0.5, 1.0], [0.6, 0.0, 0.4, 1.0], [-0.1, 0.0, 0.5, 1.0], [0.0, 0.0, 1.1, 1.0], [0.0, 0.7, 1.0, 0.7],
                                 [0.0, 0.0, 1.0, 1.5]])
def test_refuses_bad_boxes(box):
    with pytest.raises(ValueError, match="0 <= x0 < x1 <= 1"):
        _call(region_boxes=[BOXES[0], box])


def test_accepted_arguments_reach_the_device_work():
    """The legal calls pass every check and fail only where the engine is first needed."""
    with pytest.raises(AttributeError):
        _call()
    with pytest.raises(AttributeError):
        _call(region_boxes=None, region_masks=torch.zeros(2, 512, 512, dtype=torch.bool))
    with pytest.raises(AttributeError):
        _call(region_boxes=[BOXES], height=256, width=384, bootstrapping=0)
    with pytest.raises(AttributeError):                          # no foreground regions: R = 1
        _stub()(prompt_embeds=torch.zeros(2, 77, 768), region_prompts=[])


def test_check_region_args_is_shared_and_returns_the_pixel_masks():
    from agenda_amd.regions import check_region_args
    px = check_region_args("DDIMScheduler", 2, None, BOXES, 64, 128)
    assert px.shape == (2, 64, 128) and px.dtype == torch.uint8
    assert torch.equal(px, R.boxes_to_masks(BOXES, 64, 128))
    assert check_region_args("DDIMScheduler", 0, None, None, 64, 64) is None
    f = check_region_args("DDIMScheduler", 1, torch.rand(2, 1, 64, 64, dtype=torch.float64), None, 64, 64, batch=2)
    assert f.dtype == torch.float32 and f.shape == (2, 1, 64, 64)


# ---- generation.py flags --------------------------------------------------------------------------------------------------------
def test_generation_flags(tmp_path):
    from agenda_amd.generation import parse_args, region_layouts_from_args, region_records
    a = parse_args(["--synthetic-config", "tiny", "--region-prompts", "a", "b", "--region-boxes", "0", "0", ".5", "1", ".5", "0", "1", "1"])
    assert a.scheduler == "DDIMScheduler" and a.bootstrapping is None and a.region_prompts == ["a", "b"]
    lays = region_layouts_from_args(a)
    assert lays == [{"prompts": ["a", "b"], "boxes": [[0.0, 0.0, 0.5, 1.0], [0.5, 0.0, 1.0, 1.0]], "masks": None}]
    rec = region_records([0, 1], lays, 112)
    assert rec["1.png"]["boxes_px"] == [[0.0, 0.0, 56.0, 112.0], [56.0, 0.0, 112.0, 112.0]] and rec["0.png"]["prompts"] == ["a", "b"]
    a = parse_args(["--region-prompts", "a", "--region-masks", "m.png", "--bootstrapping", "5"])
    assert a.region_masks == ["m.png"] and a.bootstrapping == 5
    lay = tmp_path / "lay.json"
    lay.write_text(json.dumps([{"prompts": ["a"], "boxes": [[0, 0, 0.5, 0.5]]}, {"prompts": ["b", "c"], "boxes": [[0, 0, 1, 0.5], [0, 0.5, 1, 1]]}]))
    a = parse_args(["--region-layouts", str(lay)])
    assert [len(x["prompts"]) for x in region_layouts_from_args(a)] == [1, 2]
    box = ["--region-boxes", "0", "0", "1", "1"]
    for bad in (["--region-prompts", "a"], ["--region-prompts", "a"] + box + ["--region-masks", "m.png"], ["--region-prompts", "a", "b"] + box,
                ["--region-prompts", "a", "--region-boxes", "0", "0", "1"], ["--region-prompts", "a", "--region-boxes", ".5", "0", ".5", "1"],
                ["--region-prompts", "a", "b", "--region-masks", "m.png"], box, ["--bootstrapping", "3"],
                ["--region-prompts", "a", "--bootstrapping", "-1"] + box, ["--region-layouts", str(lay), "--region-prompts", "a"] + box,
                ["--region-prompts", "a", "--scheduler", "PNDMScheduler"] + box, ["--region-prompts", "a", "--panorama"] + box,
                ["--region-prompts", "a", "--gligen-phrases", "a", "--gligen-boxes", "0", "0", "1", "1"] + box,
                ["--region-prompts", "a", "--controlnet-model-path", "cn", "--control-image", "c.png"] + box,
                ["--region-prompts", "a", "--adapter-model-path", "ad", "--adapter-image", "c.png"] + box,
                ["--region-prompts", "a", "--ip-adapter-path", "ip", "--ip-adapter-image", "c.png"] + box,
                ["--region-prompts", "a", "--init-image", "x.png", "--mask-image", "m.png"] + box,
                ["--region-prompts", "a", "--instruct-image", "x.png"] + box, ["--region-prompts", "a", "--pag-scale", "3"] + box,
                ["--region-prompts"] + list("abcdefgh") + ["--region-boxes"] + ["0", "0", "1", "1"] * 8):
        with pytest.raises(SystemExit):
            parse_args(bad)
    plain = parse_args([])
    assert plain.region_prompts is None and plain.region_layouts is None and plain.bootstrapping is None and plain.scheduler is None


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_exported_and_bound():
    from agenda_amd import _lib
    txt = open(os.path.join(ROOT, "include", "agenda_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    so = os.path.join(ROOT, "agenda_amd", "libagenda_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} not declared in include/agenda_hip.h"
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.EXPORTS
    assert "agd_regions_desc" in txt and ctypes.sizeof(_lib.AgdRegionsDesc) == 16 + 5 * ctypes.sizeof(ctypes.c_void_p)

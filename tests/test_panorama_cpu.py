"""MultiDiffusion panorama, host side: `get_views` known answers, the restated overlap mean's coverage, every refusal of
StableDiffusionPanoramaPipeline (raised before any device work: the pipeline object here has no engine at all), generation.py's
--panorama flags, and the new C-ABI symbols."""
import ctypes
import os
import re
import types

import pytest
import torch

import _panorama_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("agd_op_window_gather", "agd_op_window_mean", "agd_denoise_panorama", "agd_daam_global_panorama")


# ---- get_views ----------------------------------------------------------------------------------------------------------------
def test_get_views_known_answers():
    from agenda_amd import StableDiffusionPanoramaPipeline, get_views
    v = get_views(512, 2048)
    assert len(v) == 25 and v[0] == (0, 64, 0, 64) and v[-1] == (0, 64, 192, 256)
    assert len(get_views(1024, 1024)) == 81
    assert get_views(512, 512) == [(0, 64, 0, 64)]
    assert len(get_views(16 * 8, 40 * 8, window_size=16)) == 4
    assert len(get_views(32 * 8, 32 * 8, window_size=16, stride=8)) == 9
    assert StableDiffusionPanoramaPipeline.get_views(512, 2048) == v
    # row-major order: view i is row i // nbw, column i % nbw
    v9 = get_views(256, 256, window_size=16)
    assert v9[1] == (0, 16, 8, 24) and v9[3] == (8, 24, 0, 16)


@pytest.mark.parametrize("lh,lw,win", [(64, 256, 64), (128, 128, 64), (16, 40, 16), (40, 16, 16), (32, 32, 16), (24, 48, 24), (40, 40, 24), (96, 192, 96)])
def test_restated_views_agree_with_the_pipeline_helper(lh, lw, win):
    from agenda_amd import get_views
    assert R.get_views(lh, lw, win) == get_views(8 * lh, 8 * lw, win, 8)


def test_restated_mean_coverage_and_constant():
    lh, lw, win = 64, 256, 64
    V = len(R.get_views(lh, lw, win))
    views = torch.full((V, 1, win, win), 3.25)
    out, count = R.overlap_mean(views, 1, lh, lw, return_count=True)
    for c in range(lw):
        assert int(count[0, 0, 0, c]) == min(c // 8 + 1, 8, (255 - c) // 8 + 1), c
    assert bool((count[0, 0] == count[0, 0, :1]).all())                # one row of views: the count does not depend on the row
    assert torch.equal(out, torch.full_like(out, 3.25))               # equal views give that constant back


def test_restated_mean_of_slices_is_the_canvas():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 32, 40, generator=g)
    back = R.overlap_mean(R.slice_views(x, 16), 2, 32, 40)
    assert torch.allclose(back, x, rtol=1e-6, atol=1e-6)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _stub(scheduler="DDIMScheduler", window=64, in_channels=4, hooker=None):
    """A pipeline object with no engine: any device work would raise AttributeError, not the refusal under test."""
    from agenda_amd import StableDiffusionPanoramaPipeline
    from agenda_amd import scheduler as S
    from agenda_amd.config import CONFIGS
    pipe = object.__new__(StableDiffusionPanoramaPipeline)
    cfg = CONFIGS["sd15"]()
    cfg.default_sample_size = window
    cfg.unet = types.SimpleNamespace(in_channels=in_channels, out_channels=4)
    pipe.cfg = cfg
    pipe.vae_scale_factor = 8
    pipe.scheduler = S.SCHEDULERS[scheduler].from_config(cfg.sched)
    pipe._hooker, pipe._trace, pipe._lora = hooker, None, None
    return pipe


@pytest.mark.parametrize("name", ["PNDMScheduler", "DPMSolverMultistepScheduler"])
def test_refuses_multistep_schedulers_by_name(name):
    with pytest.raises(ValueError) as e:
        _stub(name)("a prompt")
    assert name in str(e.value) and 'scheduler="DDIMScheduler"' in str(e.value) and "from_pretrained" in str(e.value)


def test_refuses_circular_padding():
    with pytest.raises(ValueError, match="circular_padding=True"):
        _stub()("a prompt", circular_padding=True)


@pytest.mark.parametrize("h,w,win", [(448, 2048, 64), (512, 480, 64), (512, 2040, 64), (512, 1000, 64), (128, 96, 16), (192, 200, 24), (760, 1536, 96)])
def test_refuses_sizes_below_the_window_or_off_the_stride_grid(h, w, win):
    with pytest.raises(ValueError) as e:
        _stub(window=win)("a prompt", height=h, width=w)
    assert f"height={h}" in str(e.value) and f"width={w}" in str(e.value) and str(8 * win) in str(e.value)


def test_refuses_an_installed_hooker():
    with pytest.raises(ValueError, match="UNetCrossAttentionHooker"):
        _stub(hooker=object())("a prompt")


def test_refuses_an_inpainting_unet():
    with pytest.raises(ValueError) as e:
        _stub(in_channels=9)("a prompt")
    assert "9 input channels" in str(e.value)


@pytest.mark.parametrize("vb", [0, -1, 2.5])
def test_refuses_bad_view_batch_size(vb):
    with pytest.raises(ValueError) as e:
        _stub()("a prompt", view_batch_size=vb)
    assert repr(vb) in str(e.value)


def test_accepted_arguments_reach_the_device_work():
    """The legal default call passes every check and fails only where the engine is first needed."""
    with pytest.raises(AttributeError):
        _stub()("a prompt", prompt_embeds=torch.zeros(2, 77, 768))


# ---- generation.py --panorama ---------------------------------------------------------------------------------------------------
def test_generation_flags():
    from agenda_amd.generation import parse_args
    a = parse_args(["--panorama"])
    assert (a.height, a.width, a.scheduler, a.view_batch_size) == (512, 2048, "DDIMScheduler", None)
    a = parse_args(["--panorama", "--synthetic-config", "tiny", "--height", "128", "--width", "320", "--view-batch-size", "2"])
    assert (a.height, a.width, a.view_batch_size) == (128, 320, 2)
    for bad in (["--panorama", "--scheduler", "PNDMScheduler"], ["--panorama", "--height", "448"], ["--panorama", "--width", "256"],
                ["--panorama", "--view-batch-size", "0"], ["--view-batch-size", "2"],
                ["--panorama", "--gligen-phrases", "a", "--gligen-boxes", "0", "0", "1", "1"],
                ["--panorama", "--init-image", "x.png", "--mask-image", "m.png"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    plain = parse_args([])
    assert plain.panorama is False and plain.height is None and plain.width is None and plain.scheduler is None


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

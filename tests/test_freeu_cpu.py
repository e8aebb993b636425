"""FreeU without a GPU: the rank-4 moment form the device kernel computes against the torch.fft restatement (tests/_freeu_restated.py), the
restated UNet walk against the oracle (all four parameters 1: bit for bit) and how far FreeU moves it, the CLI flag, and the C ABI."""
import os
import re

import pytest
import torch

import _freeu_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (3, 3), (4, 4), (8, 8), (9, 8), (16, 16), (6, 4), (32, 24)]


def _rms_rel(got, want):
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("s", [0.2, 0.9])
def test_moment_form_equals_the_fft_filter(H, W, s):
    """fp64 both ways: the filter touches the frequencies {-1 mod H, 0} x {-1 mod W, 0} as sets (a side of 1 or 2 included)."""
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn(2, 5, H, W, generator=g, dtype=torch.float64)
    want = R.fourier_filter(x, 1, s)
    got = R.fourier_filter_moments(x, s)
    err = float((got - want).abs().max())
    assert err < 1e-12 * max(1.0, float(want.abs().max())) * H * W, err
    if H * W == 1:
        assert torch.allclose(want, s * x, atol=1e-14)               # frequency 0 alone, scaled once


def test_filter_in_fp32_against_fp64():
    """What the issue measured: the fp32 torch.fft form and the fp64 moment form agree to about 6e-7 (unit-variance maps)."""
    worst = 0.0
    for H, W in SIZES:
        for s in (0.2, 0.9):
            g = torch.Generator().manual_seed(7 * H + W)
            x = torch.randn(2, 3, H, W, generator=g)
            worst = max(worst, float((R.fourier_filter(x, 1, s).double() - R.fourier_filter_moments(x.double(), s)).abs().max()))
    print(f"fp32 fft filter vs fp64 moment form: max abs {worst:.2e}")
    assert worst < 5e-6, worst


def test_apply_freeu_touches_what_it_should():
    g = torch.Generator().manual_seed(1)
    h, sk = torch.randn(2, 10, 4, 6, generator=g), torch.randn(2, 6, 4, 6, generator=g)
    for idx, (b, s) in enumerate([(1.5, 0.9), (1.6, 0.2)]):
        ho, so = R.apply_freeu(idx, h, sk, 0.9, 0.2, 1.5, 1.6)
        assert torch.equal(ho[:, :5], h[:, :5] * b) and torch.equal(ho[:, 5:], h[:, 5:])
        assert torch.allclose(so, R.fourier_filter(sk, 1, s))
        assert torch.allclose(so.mean((-2, -1)), s * sk.mean((-2, -1)), atol=1e-6)      # the mean is frequency (0, 0)
    ho, so = R.apply_freeu(2, h, sk, 0.9, 0.2, 1.5, 1.6)
    assert ho is h and so is sk


# config, latent height, latent width, the rms-rel distance measured for (0.9, 0.2, 1.5, 1.6)
CPU_CASES = [("tiny", 16, 16, 0.327), ("tiny21", 24, 24, 0.366), ("tiny", 16, 24, 0.323), ("tiny40", 16, 16, 0.645)]
_PLAIN = {}


def _setup(name, Lh, Lw):
    """The GPU tests' forward: two rows, t = 301; the plain oracle forward is computed once per case and shared."""
    from agenda_amd import config, synthetic
    from oracle import sd_oracle as O
    key = (name, Lh, Lw)
    if key not in _PLAIN:
        cfg = config.CONFIGS[name]()
        u = synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1)
        ctx = synthetic.make_context(cfg, 1, seed=6)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(2, 4, Lh, Lw, generator=g)
        t = torch.tensor(301.0)
        with torch.no_grad():
            plain = O.unet_forward(u, cfg.unet, x, t, ctx)
        _PLAIN[key] = (cfg, u, ctx, x, t, plain)
    return _PLAIN[key]


@pytest.mark.parametrize("name,Lh,Lw,measured", CPU_CASES)
def test_restated_walk_against_the_oracle(name, Lh, Lw, measured):
    """All four parameters 1: the re-walk IS the oracle's forward, bit for bit.  With the suggested SD-1.5 values, with the filter alone and
    with the backbone scale alone it moves by far more than the 0.03 bound the GPU tests hold the engine to -- the distance a missing or
    half-applied FreeU would show there."""
    cfg, u, ctx, x, t, plain = _setup(name, Lh, Lw)
    with torch.no_grad():
        assert torch.equal(R.unet_forward_with_freeu(u, cfg.unet, x, t, ctx, 1, 1, 1, 1), plain)
        full = R.unet_forward_with_freeu(u, cfg.unet, x, t, ctx, 0.9, 0.2, 1.5, 1.6)
        filt = R.unet_forward_with_freeu(u, cfg.unet, x, t, ctx, 0.9, 0.2, 1, 1)
        back = R.unet_forward_with_freeu(u, cfg.unet, x, t, ctx, 1, 1, 1.5, 1.6)
    d = [_rms_rel(plain, w) for w in (full, filt, back)]
    print(f"restated FreeU {name} {Lh}x{Lw}: the plain forward is {d[0]:.3f} (filter only {d[1]:.3f}, backbone only {d[2]:.3f}) rms-rel away")
    assert d[0] == pytest.approx(measured, abs=0.02), d
    assert min(d) > 0.12, d


def test_generation_cli_freeu_flag():
    from agenda_amd import generation
    assert generation.parse_args([]).freeu is None
    a = generation.parse_args(["--freeu", "0.9", "0.2", "1.5", "1.6"])
    assert a.freeu == [0.9, 0.2, 1.5, 1.6]
    # beside the other pipelines' flags
    a = generation.parse_args(["--freeu", "0.9", "0.2", "1.2", "1.4", "--panorama", "--synthetic-config", "tiny", "--scheduler", "DDIMScheduler"])
    assert a.freeu == [0.9, 0.2, 1.2, 1.4] and a.panorama
    a = generation.parse_args(["--scheduler", "PNDMScheduler", "--freeu", "1", "1", "1", "1", "--height", "128", "--width", "192"])
    assert a.freeu == [1.0] * 4 and (a.height, a.width) == (128, 192)
    for bad in (["--freeu", "0.9", "0.2", "1.5"], ["--freeu", "0.9", "0.2", "1.5", "1.6", "2.0"], ["--freeu"],
                ["--freeu", "0.9", "0.2", "nan", "1.6"], ["--freeu", "inf", "0.2", "1.5", "1.6"], ["--freeu", "a", "0.2", "1.5", "1.6"]):
        with pytest.raises(SystemExit):
            generation.parse_args(bad)


FREEU_SYMBOLS = ("agd_freeu_set", "agd_freeu_clear", "agd_freeu_counts", "agd_op_freeu")


def test_library_exports_every_freeu_symbol():
    import ctypes
    from agenda_amd import _lib
    so = os.path.join(ROOT, "agenda_amd", "libagenda_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    txt = open(os.path.join(ROOT, "include", "agenda_hip.h")).read()
    for s in FREEU_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} not declared in include/agenda_hip.h"
        assert s in _lib.EXPORTS


def test_python_surface():
    """enable_freeu / disable_freeu on the pipeline and on pipe.unet (every subclass inherits them), the engine methods and ops.freeu."""
    import agenda_amd
    from agenda_amd import ops, pipeline
    for cls in (pipeline.StableDiffusionPipeline, pipeline.UNetHandle):
        assert callable(getattr(cls, "enable_freeu")) and callable(getattr(cls, "disable_freeu"))
    for name in ("freeu_set", "freeu_clear", "freeu_counts"):
        assert callable(getattr(pipeline.Engine, name))
    assert callable(ops.freeu)
    for sub in ("StableDiffusionControlNetPipeline", "StableDiffusionInpaintPipeline", "StableDiffusionInstructPix2PixPipeline",
                "StableDiffusionPanoramaPipeline", "StableDiffusionAdapterPipeline", "StableDiffusionGLIGENPipeline"):
        cls = getattr(agenda_amd, sub)
        assert cls.enable_freeu is pipeline.StableDiffusionPipeline.enable_freeu, sub

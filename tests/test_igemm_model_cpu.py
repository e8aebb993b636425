"""tests/_igemm_model.py checked on its own, without a GPU: the reference's pieces against independent formulations in fp64, every case of the
shared lists against the conditions a kernel may be judged under (ceiling, residual condition, LayerNorm rows), the kernel family every case
expects against launch_igemm's shape rules restated by hand, and the measures against deliberately wrong models -- the errors the GPU tests are
there to catch."""
import math

import pytest
import torch
import torch.nn.functional as F
import _igemm_model as IM
from _norm_model import gn_slabs, groupnorm_fp64, slab_errors

ALL = IM.LAUNCHED
REFUSED = [c for c, _ in IM.SHORTCUT_REFUSED + IM.COLSTAT_REFUSED + IM.WPI_REFUSED]


# ------------------------------------------------------------------------------------------------------------------------------
# the reference against other formulations
# ------------------------------------------------------------------------------------------------------------------------------
def _im2col(c, x):
    """[images, H, W, C] -> [M, taps * C] in the kernel's K order (tap-major), through F.unfold (channel-major) and a permutation"""
    t = x.permute(0, 3, 1, 2).double()
    if c["up"] == 2:
        t = t.repeat_interleave(2, 2).repeat_interleave(2, 3)
    k = c["ksize"]
    if c["asym"]:
        t, pad, stride = F.pad(t, (0, 1, 0, 1)), 0, 2
    else:
        pad, stride = (1 if k == 3 else 0), c["stride"]
    cols = F.unfold(t, k, padding=pad, stride=stride)                   # [B, C * k * k, L], rows ordered (channel, tap)
    B, _, L = cols.shape
    return cols.reshape(B, t.shape[1], k * k, L).permute(0, 3, 2, 1).reshape(B * L, -1)


@pytest.mark.parametrize("name", ["g64 1x1 cat 64|128", "g64 3x3 cat 64|128", "g64 3x3 stride 2 cat 192|64", "g64 3x3 up 2 cat 64|128", "g64 asymmetric odd",
                                  "sc smap split two sources residual", "8p 160 wide stride 2 cat"])
def test_the_gather_is_a_matrix_product_in_the_kernels_k_order(name):
    """conv(cat(src0, src1)) (+ conv1x1(cat(sc0, sc1))) = [im2col | shortcut rows] . kernel_matrix^T: the concat gather is the conv on the
    concatenated tensor, the shortcut fold is extra K, and `kernel_matrix` states the K order the launch is handed"""
    c = IM.BY_NAME[name]
    i = IM.inputs(c)
    x, sc = IM._sources(c, i)
    a = _im2col(c, x)
    if sc is not None:
        a = torch.cat([a, sc.double().reshape(a.shape[0], -1)], 1)
    w = IM.kernel_matrix(c, i)[0].double()
    assert a.shape == (IM.dims(c)[0], IM.dims(c)[3])
    want = IM._acc(c, i, torch.float64)
    assert float((a @ w.T - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_the_asymmetric_pad_pads_bottom_and_right():
    c = IM.BY_NAME["g64 asymmetric odd"]
    i = IM.inputs(c)
    x = torch.cat([i["x0"], i["x1"]], -1).double()
    w = i["w4"][0].double()
    want = IM._acc(c, i, torch.float64).reshape(c["images"], c["H"] // 2, c["W"] // 2, -1)
    for (b, oy, ox) in ((0, 0, 0), (1, c["H"] // 2 - 1, c["W"] // 2 - 1), (0, c["H"] // 2 - 1, 2)):
        acc = torch.zeros(c["N"], dtype=torch.float64)
        for ky in range(3):
            for kx in range(3):
                y, xx = 2 * oy + ky, 2 * ox + kx                           # no top / left padding: tap (0, 0) is the pixel itself
                if y < c["H"] and xx < c["W"]:
                    acc += w[:, :, ky, kx] @ x[b, y, xx]
        assert float((acc - want[b, oy, ox]).abs().max()) <= 1e-12 * float(want.abs().max())
    other = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (1, 0, 1, 0)), w, stride=2).permute(0, 2, 3, 1)
    assert float((other - want).abs().max()) > 0.1 * float(want.abs().max()), "the other phase must be a different function"


@pytest.mark.parametrize("name", ["ln general one slot", "ln general geglu", "ln general offset rows"])
def test_the_layernorm_fold_identity(name):
    """rstd (x W'^T - mu cs) + b' with W' = W gamma, cs = its column sums, b' = b + W beta is layer_norm(x) W^T + b -- exactly, before W' is rounded"""
    c = IM.BY_NAME[name]
    i = IM.inputs(c)
    M, N, Nout, K, HWo = IM.dims(c)
    x = i["x0"].double().reshape(M, -1)
    w = i["w4"][0].reshape(N, -1).double()
    wf, b = w * i["gamma"].double()[None], i["bias"].double() + w @ i["beta"].double()
    mu, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    rstd = (var + float(torch.tensor(IM.LN_EPS, dtype=torch.float32))).rsqrt()
    folded = rstd * (x @ wf.T - mu * wf.sum(1)[None]) + b[None]
    want = IM._pre(c, i, False)
    assert float((folded - want).abs().max()) <= 1e-11 * float(want.abs().max())
    # ... and the table the consumer is handed adds up to the rows' sums
    t = IM.ln_table(c, i).double().sum(1)
    assert float((t[:, 0] - x.sum(1)).abs().max()) <= 2.0 ** -20 * float(x.abs().sum(1).max())
    assert float((t[:, 1] - x.pow(2).sum(1)).abs().max()) <= 2.0 ** -20 * float(x.pow(2).sum(1).max())


def test_the_geglu_is_value_times_gelu_of_gate():
    c = IM.BY_NAME["ln general geglu"]
    v = IM._pre(c, IM.inputs(c), False)
    want = v[:, :128] * F.gelu(v[:, 128:])
    assert float((IM.igemm_fp64(c) - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_the_activations_and_the_epilogue_order():
    c = IM.BY_NAME["general vector all together"]
    i = IM.inputs(c)
    M, N, Nout, K, HWo = IM.dims(c)
    acc = i["x0"].double().reshape(M, -1) @ i["w4"][0].reshape(N, -1).double().T
    pre = 0.5 * acc + i["bias"].double()[None] + i["rowadd"].double().repeat_interleave(HWo, 0) + i["res"].double()[:, :N]
    assert float((IM.igemm_fp64(c) - F.silu(pre)).abs().max()) <= 1e-12 * float(pre.abs().max())
    t = torch.linspace(-6, 6, 97, dtype=torch.float64)
    assert torch.allclose(IM._act64(t, 2), t / (1 + torch.exp(-1.702 * t)), rtol=1e-14, atol=0)
    assert torch.allclose(IM._act64(t, 3), F.gelu(t), rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=[c["name"] for c in ALL])
def test_cases_satisfy_their_conditions(c):
    IM.check_case_conditions(c)
    M, N, Nout, K, HWo = IM.dims(c)
    assert K % 64 == 0 and c["C0"] % 64 == 0 and c["C1"] % 64 == 0
    t, kw = IM.launch_args(c)
    assert t["w"].shape[-1] == K and t["w"].shape[-2] == N


def test_inputs_tell_images_sources_and_channel_blocks_apart():
    c = IM.BY_NAME["halo Wout 32 cat 64|128"]
    i = IM.inputs(c)
    m0 = i["x0"].double().mean((1, 2, 3))
    assert float((m0[:, None] - m0[None, :]).abs().add(torch.eye(3)).min()) > 0.1, "every image its own offset"
    assert abs(float(i["x1"].double()[..., :64].mean() - i["x1"].double()[..., 64:].mean())) > 0.1, "every channel block its own offset"
    assert float(i["x1"].double().std() / i["x0"].double().std()) > 1.2, "every source its own scale"


# launch_igemm's shape rules, restated by hand (csrc/igemm.hip at this commit; nk = K / 64, t128 = ceil(M / 128) ceil(N / 128) batch):
#   shortcut sources            a 3x3 launch that halo_ok() or the 8 x 8 whole-images kernel takes, else refused
#   w_per_image                 N % 160 == 0 and (M / 64)(N / 160) <= 256: 64 x 160 (pc bit 0: the pc kernel); images of hw % 128 != 0 rows: 64 x 64
#   pc bit 1 / bit 3 (3x3)      N % 160 == 0, M % 64 == 0, t64 = (M / 64)(N / 160): bit 1 at 192 <= t64 <= 256 unsplit; bit 3 at t64 <= 64, nk >= 64:
#                               min(256 / t64, 8, nk / 16) slices
#   smap (8 x 8 maps, 3x3)      tiles = ceil(M / 512)(N / 64), chunks = (C0 + C1) / 64, slices = the chunks spread over min(256 / tiles, chunks)
#   wreg                        1x1 single source bf16, ceil(M / 64)(N / BN) >= 128 tiles: BN = 256 (GEGLU), 160 where that fills one wave, else 128
#   p8 = 2 / 3                  3x3 or plain 1x1, no rowstat producer: the 256- / 160-wide 256-row tile
#   GEGLU                       128 x 128
#   1x1, N % 160 == 0, M % 64 == 0, nk >= 16   t64 in 192 .. 256: 64 x 160 (pc bit 0: pc); t64 <= 64, nk >= 64, may split: min(256 / t64, nk / 16) slices
#   t128 <= 160, nk >= 64, M >= 128            128-row tiles on the deep ring, slices = min(256 / tiles, 8, nk / 8) (1 for statistics producers /
#                                              consumers), 160-wide where that gives more workgroups
#   N <= 64                     64 x 64
#   t128 >= 192                 128 x 160 where N % 160 == 0 and N % 128 != 0 (64 x 160 for <= 128 deep-ring tiles of a non-halo launch), else 128 x 128
#   otherwise                   64 x 64
#   128-row unsplit or split 3x3 tiles with `halo` and halo_ok(): the row-halo kernel (pc bit 4 and <= 256 workgroups on 160-wide tiles: pch)
#   a split launch is followed by the plain slab pass, or the GroupNorm one where reduce_gn_ok()
G64, G128, G160, G64x160 = ("general", "none", (64, 64, 1)), ("general", "none", (128, 128, 1)), ("general", "none", (128, 160, 1)), ("general", "none", (64, 160, 1))
HALO160, PC160 = ("halo", "none", (128, 160, 1)), ("pc", "none", (64, 160, 1))
EXPECTED = {
    "g64 1x1 cat 64|128": G64, "g64 1x1 cat 192|64": G64, "g64 3x3 cat 64|128": G64, "g64 3x3 stride 2 cat 192|64": G64, "g64 3x3 up 2 cat 64|128": G64,
    "g64 asymmetric even": G64, "g64 asymmetric odd": G64, "g64 3x3 eight images": G64,
    "g128x128 two stages cat": G128, "g128x128 four stages cat": G128, "g128x160 two stages": G160, "g64x160 deep ring cat": G64x160,
    "g64x160 3x3 without halo": G64x160,
    "halo Wout 16": HALO160, "halo Wout 32 cat 64|128": HALO160, "halo Wout 64": HALO160, "halo Wout 128": HALO160, "halo Wout 256": HALO160, "halo up 2": HALO160,
    "pch Wout 64": ("pch", "none", (128, 160, 1)), "pc 3x3 cat 64|64": PC160,
    "8p 256 wide cat": ("8p", "none", (256, 256, 1)), "8p 160 wide stride 2 cat": ("8p", "none", (256, 160, 1)),
    "smap unsplit": ("smap", "none", (512, 64, 1)), "smap cat 64|64 split": ("smap", "plain", (512, 64, 2)),
    "sc halo one source": HALO160, "sc halo two sources residual rowadd": HALO160,
    "sc halo split": ("halo", "plain", (128, 128, 8)), "sc halo split two sources residual rowadd": ("halo", "plain", (128, 128, 8)),
    "sc smap": ("smap", "none", (512, 64, 1)), "sc smap split two sources residual": ("smap", "plain", (512, 64, 2)),
    "slab general linear forms": ("general", "plain", (64, 160, 4)), "slab general all forms": ("general", "plain", (64, 160, 4)),
    "slab general N 320 linear forms": ("general", "plain", (64, 160, 5)), "slab general N 320 odd pitch": ("general", "plain", (64, 160, 5)),
    "slab general N 320 all forms odd pitch": ("general", "plain", (64, 160, 5)), "slab general N 320 row bias quick gelu": ("general", "plain", (64, 160, 5)),
    "slab general N 320 gelu": ("general", "plain", (64, 160, 5)),
    "slab halo all forms": ("halo", "plain", (128, 128, 8)), "slab halo linear forms": ("halo", "plain", (128, 128, 8)),
    "slab pc all forms": ("pc", "plain", (64, 160, 4)), "slab pc linear forms": ("pc", "plain", (64, 160, 4)),
    "slab smap all forms": ("smap", "plain", (512, 64, 2)), "slab smap linear forms": ("smap", "plain", (512, 64, 2)),
    "batched shared A row bias": G64, "batched scores alpha fp32": G64, "batched P V^T": G64,
    "rowstat one slot": G128, "rowstat two slots 160 wide": G160, "rowstat three slots ragged tile": G128, "rowstat 64 wide tiles": G64, "rowstat pc": PC160,
    "rowstat wreg": ("wreg", "none", (64, 128, 1)), "rowstat 8p declines": G64,
    "ln general one slot": G64, "ln general two slots element": G64, "ln general three slots mean 1 std 3": G64, "ln general offset rows": G64,
    "ln general geglu": G128, "ln general geglu element": G128, "ln pc": PC160, "ln wreg": ("wreg", "none", (64, 128, 1)),
    "ln wreg geglu": ("wreg", "none", (64, 256, 1)), "ln 8p": ("8p", "none", (256, 256, 1)),
    "colstat 1x1": G64, "colstat halo": ("halo", "none", (128, 128, 1)), "colstat pc": PC160, "colstat wreg": ("wreg", "none", (64, 128, 1)),
    "colstat 8p": ("8p", "none", (256, 256, 1)),
    "gn 640 quads": ("general", "gn", (64, 160, 4)), "gn 640 quads all forms": ("general", "gn", (64, 160, 4)), "gn 704 quads no bias": ("general", "gn", (128, 128, 8)),
    "gn 1280 quads rowadd": ("general", "gn", (64, 160, 4)), "gn 2560 quads residual": ("general", "gn", (64, 160, 4)),
    "gn declined: 42 channels per group": ("general", "plain", (128, 128, 8)), "gn declined: 3328 quads": ("general", "plain", (128, 128, 8)),
    "gn declined: quick gelu": ("general", "plain", (64, 160, 4)), "gn declined: fp32 output": ("general", "plain", (64, 160, 4)),
    "wpi 64x160": G64x160, "wpi 64x160 pc": PC160, "wpi 64-row images": G64, "wpi 128-row tiles": G128,
}
# the generated epilogue cases: M = 192, N = 200 or 72, K = 128 -- none of the wide-tile rules applies
EXPECTED.update({c["name"]: G64 for c in IM.EPILOGUE if c["name"].startswith("general ")})
# the forms on the other families' shapes: M = 12288, N = 160, 3x3 with `halo` (192 tiles of 128 x 128 -> 128 x 160, halo_ok); M = 1536, N = 1280,
# K = 1024 with pc bit 0 (t64 = 24 x 8 = 192); M = 512, N = 256 with p8 = 2; M = 1024, N = 1024 bf16 with wreg (16 x 8 = 128 tiles of 64 x 128)
for _fam, _exp in (("halo", HALO160), ("pc", PC160), ("8p", ("8p", "none", (256, 256, 1))), ("wreg", ("wreg", "none", (64, 128, 1)))):
    EXPECTED.update({c["name"]: _exp for c in IM.EPILOGUE if c["name"].startswith(_fam + " ")})


def test_every_case_expects_the_family_the_shape_rules_give():
    assert set(EXPECTED) == set(IM.BY_NAME), sorted(set(EXPECTED) ^ set(IM.BY_NAME))
    for name, (family, slab, cfg) in EXPECTED.items():
        c = IM.BY_NAME[name]
        assert (c["family"], c["slab"], tuple(c["cfg"])) == (family, slab, cfg), name
    for c in REFUSED:
        assert (c["family"], c["slab"]) == ("none", "none")
    families = {c["family"] for c in ALL}
    assert families == {"general", "halo", "pch", "pc", "8p", "smap", "wreg"}, families
    assert {c["slab"] for c in ALL} == {"none", "plain", "gn"}


def test_the_tile_arithmetic_behind_the_table():
    """the numbers the table above rests on, for the cases that sit on a threshold"""
    def t128(c):
        M, N = IM.dims(c)[:2]
        return math.ceil(M / 128) * math.ceil(N / 128)
    for name in ("halo Wout 16", "halo Wout 256", "halo up 2", "g128x160 two stages", "g128x128 two stages cat", "rowstat two slots 160 wide"):
        assert t128(IM.BY_NAME[name]) == 192, name                          # the first launch that takes 128-row tiles without a long K
    for name, t64, s in (("slab general linear forms", 64, 4), ("slab general N 320 linear forms", 16, 5), ("gn 640 quads", 2, 4), ("gn 1280 quads rowadd", 8, 4)):
        c = IM.BY_NAME[name]
        M, N, _, K, _ = IM.dims(c)
        assert (M // 64) * (N // 160) == t64 and min(256 // t64, K // 64 // 16) == s == c["cfg"][2], name
    for name in ("pc 3x3 cat 64|64", "pc linear forms together", "wpi 64x160"):
        M, N = IM.dims(IM.BY_NAME[name])[:2]
        assert 192 <= (M // 64) * (N // 160) <= 256, name
    for c in IM.SLAB_GN:
        M, N, _, _, HWo = IM.dims(c)
        q = HWo * (N // c["gn"]["groups"] // 4)
        assert q == int(c["name"].split()[1]) and q <= 3072 and (N // c["gn"]["groups"]) % 4 == 0


# ------------------------------------------------------------------------------------------------------------------------------
# the measures against wrong models: what a kernel error of each kind would look like
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation,name", [
    ("swap_sources", "8p 256 wide cat"), ("swap_sources", "smap cat 64|64 split"),
    ("rowadd_next_image", "general vector rowadd"), ("rowadd_next_image", "general vector all together"),
    ("act_before_residual", "general vector all together"), ("act_before_residual", "slab general all forms"),
    ("drop_chunk", "g64 1x1 cat 192|64"), ("drop_chunk", "slab general linear forms"), ("drop_chunk", "halo all together"),
    ("bias_n_for_mode2", "general vector row bias"), ("bias_n_for_mode2", "batched shared A row bias"),
    ("skip_slab", "slab general N 320 linear forms"), ("skip_slab", "slab smap all forms"),
])
def test_the_bounds_reject_a_wrong_model(mutation, name):
    c = IM.BY_NAME[name]
    assert not IM.errors(c, IM.igemm_model(c))["violations"], "the model itself must be inside its bounds"
    e = IM.errors(c, IM.igemm_model(c, mutate=mutation))
    print(mutation, name, e)
    assert e["violations"], (mutation, name, e)


def test_groupnorm_statistics_taken_before_the_rounding():
    """The seventh mutation, said honestly: statistics from the un-rounded activation move mean and rstd by about 2^-9 / sqrt(elements of the
    group) relative -- orders of magnitude below a bf16 step of the output.  Neither the slab bound (MODEL_FACTOR x the model's error, itself
    half a bf16 step) nor the comparison with the separate path (one bf16 step on < 2 % of the elements) can see it reliably; what does is the
    bit-for-bit comparison `gn_keep_out`: `out` equals the plain slab pass -- together with gn_y being the GroupNorm of exactly that `out` under
    the slab bound.  This test records the sizes."""
    c = IM.BY_NAME["gn 640 quads"]
    i = IM.inputs(c)
    M, N, Nout, K, HWo = IM.dims(c)
    g = c["gn"]["groups"]
    exact = IM.igemm_fp64(c)
    act = IM._r(exact)
    nchw = lambda t: t.reshape(c["images"], HWo, N).transpose(1, 2)          # noqa: E731
    want = groupnorm_fp64(nchw(act), None, g, i["gn_gamma"], i["gn_beta"], IM.GN_EPS, True)
    model = nchw(IM.gn_model(c, act))
    # the mutation: mean / rstd from the un-rounded values, applied to the rounded ones
    xs, xr = nchw(exact).reshape(c["images"], g, -1), nchw(act).reshape(c["images"], g, -1)
    mean, var = xs.mean(-1, keepdim=True), xs.var(-1, unbiased=False, keepdim=True)
    cpg = N // g
    ga, be = i["gn_gamma"].double().reshape(1, g, cpg, 1), i["gn_beta"].double().reshape(1, g, cpg, 1)
    y = ((xr - mean) * (var + IM.GN_EPS).rsqrt()).reshape(c["images"], g, cpg, HWo) * ga + be
    bad = IM._r(y * torch.sigmoid(y)).reshape(c["images"], N, HWo)
    em = float(slab_errors(gn_slabs(model, g), gn_slabs(want, g), gn_slabs(model, g))[0].max())
    eb = float(slab_errors(gn_slabs(bad, g), gn_slabs(want, g), gn_slabs(model, g))[0].max())
    flips = float((bad != model).double().mean())
    print(f"statistics before the rounding: slab max {eb:.6f} against the model's {em:.6f}; {flips:.5f} of the elements differ from the model")
    assert eb <= IM.MODEL_FACTOR * em, "if this ever fails the slab bound DOES see the mutation: say so in the docstring"
    assert 0 < flips < 0.05, "the mutation moves isolated elements by one bf16 step, as a second correct kernel also would"

"""The implicit-GEMM launcher (csrc/igemm.hip `launch_igemm`) one launch at a time, through `agd_op_igemm`: every gather form (channel concat,
3x3, stride 2, nearest 2x, the asymmetric pad-0 form, the conv_shortcut folded as extra K), every epilogue form (alpha, the two bias modes, rowadd,
residual with its own pitch, an output pitch wider than N, the three activations, bf16 and fp32 output) on the epilogue's vector path, its
element-by-element path and the plain slab pass, the batched launches of the VAE attention, both sides of the LayerNorm fold, the GroupNorm
statistics producer, the fused slab-sum + GroupNorm pass, per-image weights, and the launcher's refusals.

Reference, model, bounds and case lists: tests/_igemm_model.py (fp64 on the bf16-rounded inputs; the fp32 bound is the standard one of an fp32
sum, the bf16 bound MODEL_FACTOR x the rounding model's own distance from fp64 per 16-row slab of one lane group's columns).

Every case asserts the kernel family and slab pass the launcher reports (`IgemmP::ran`) and the tile configuration `igemm_query` gives: a case
that falls back to another kernel fails.  Every output buffer is pre-filled with a sentinel: columns >= Nout of a row and rows >= M must keep
it.  Every split-K result is launched twice and compared bit for bit.  Refusals are host-side returns: -1, a message, the sentinel intact; no
test launches a form that is expected to fault.

Not asserted here: `colstat_out` on a split launch (the launcher never splits a statistics producer, so that refusal cannot be reached through
it).  The VAE attention's P V^T launch contracts over the tokens and the launcher takes K in multiples of 64 only: it runs 80 query rows
against 128 keys."""
import functools

import pytest
import torch
import _igemm_model as IM
from _norm_model import gn_slabs, groupnorm_fp64, slab_errors
from _report import report
from _igemm_model import MODEL_FACTOR

pytestmark = pytest.mark.gpu
IM_SENTINEL = -24576.0          # agenda_amd.ops.IGEMM_SENTINEL, asserted equal in `ops()` below


@pytest.fixture(scope="module")
def ops():
    from agenda_amd import ops as o
    assert o.IGEMM_SENTINEL == IM_SENTINEL
    return o


def ids(cases):
    return [c[0]["name"] if isinstance(c, tuple) else c["name"] for c in cases]


def launch(ops, c, check=True, **over):
    t, kw = IM.launch_args(c)
    M, N, Nout, K, HWo = IM.dims(c)
    if c["rowstat"]:
        kw["rowstat_slots"] = c["rowstat"]
    if c["colstat"]:
        kw["colstat_rows"] = HWo
    no_gn, keep_out = over.pop("no_gn", False), over.pop("keep_out", 1)
    gn = None
    if c["gn"] and not no_gn:
        gn = dict(c["gn"], gamma=t["gn_gamma"].cuda(), beta=t["gn_beta"].cuda(), eps=IM.GN_EPS, keep_out=keep_out)
    kw.update(over)
    dev = {k: (None if v is None else v.cuda()) for k, v in t.items() if k not in ("gn_gamma", "gn_beta")}
    r = ops.igemm(dev.pop("src0"), dev.pop("w"), gn=gn, check=False, **dev, **kw)
    if r["rc"] != 0 and "the launch failed" in r["err"]:        # a kernel fault: nothing else of this session may run on the device
        pytest.exit(f"igemm[{c['name']}]: {r['err']}", returncode=1)
    if check:
        assert r["rc"] == 0, (c["name"], r["err"])
    return r


def result(ops, c, r):
    """the launch's report and the sentinel -> the [rows, Nout] result (batched: the batch rows stacked)"""
    M, N, Nout, K, HWo = IM.dims(c)
    assert r["rc"] == 0, r["err"]
    assert (r["family"], r["slab"]) == (c["family"], c["slab"]), (c["name"], r["family"], r["slab"], r["cfg"])
    assert tuple(r["cfg"]) == tuple(c["cfg"]), (c["name"], r["cfg"])
    out, S = r["out"], ops.IGEMM_SENTINEL
    if c["batched"]:
        B, ldo = c["batched"]["B"], Nout + c["ldo_extra"]
        body = out[:B * M * ldo].view(B * M, ldo)
        assert bool((out[B * M * ldo:] == S).all()), "rows >= M were written"
    else:
        body = out[:M]
        assert bool((out[M:] == S).all()), "rows >= M were written"
    assert bool((body[:, Nout:] == S).all()), "columns >= Nout of a row were written"
    return body[:, :Nout]


def judge(c, got, tag=""):
    e = IM.errors(c, got)
    name = c["name"] + tag
    if c["out_f32"]:
        print(f"igemm[{name}]: worst |error| / fp32 bound {e['worst_over_bound']:.4f}")
        report(f"igemm_ops[{name}]", worst_over_bound=e["worst_over_bound"])
    else:
        print(f"igemm[{name}]: worst slab max {e['kernel_max']:.6f} (E_model {e['model_max']:.6f}), rms {e['kernel_rms']:.6f} (E_rms {e['model_rms']:.6f})")
        report(f"igemm_ops[{name}]", kernel_max=e["kernel_max"], model_max=e["model_max"], kernel_rms=e["kernel_rms"], model_rms=e["model_rms"])
    assert not e["violations"], (name, e)
    return e


def run_and_judge(ops, c, twice=False):
    r = launch(ops, c)
    got = result(ops, c, r)
    judge(c, got)
    if twice or c["cfg"][2] > 1:
        r2 = launch(ops, c)
        assert torch.equal(r["out"], r2["out"]), "a second launch of the same problem differs"
    return r, got


def refused(ops, c, word, **over):
    r = launch(ops, c, check=False, **over)
    print(f"igemm[{c['name']}]: rc {r['rc']} '{r['err']}'")
    assert r["rc"] == -1 and word in r["err"], (c["name"], r["rc"], r["err"])
    assert (r["family"], r["slab"]) == ("none", "none"), "something was launched"
    torch.cuda.synchronize()
    assert bool((r["out"] == ops.IGEMM_SENTINEL).all()), "the output was touched"
    for k in ("gn_y", "rowstat", "colstat"):
        assert k not in r or bool((r[k] == ops.IGEMM_SENTINEL).all()), k
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# gather forms
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", IM.GATHER, ids=ids(IM.GATHER))
def test_gather_forms(ops, c):
    run_and_judge(ops, c)


@pytest.mark.parametrize("name", IM.CONCAT_PAIRS)
def test_concat_is_the_single_source_of_the_same_total(ops, name):
    """src0 | src1 against ONE source holding the concatenated channels: both inside the bound, and within twice the bound of each other"""
    c = IM.BY_NAME[name]
    i = IM.inputs(c)
    a = result(ops, c, launch(ops, c))
    single = dict(c, name=name + " as one source", C0=c["C0"] + c["C1"], C1=0)
    IM._INPUTS[single["name"]] = dict({k: v for k, v in i.items() if k != "x1"}, x0=torch.cat([i["x0"], i["x1"]], -1))
    b = result(ops, single, launch(ops, single))
    bound = IM.reference(c)["bound"]
    judge(c, a)
    judge(c, b, " as one source")
    assert bool(((a - b).abs().double().cpu() <= 2 * bound).all())


# ------------------------------------------------------------------------------------------------------------------------------
# conv_shortcut folded as extra K
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", IM.SHORTCUT, ids=ids(IM.SHORTCUT))
def test_shortcut_fold(ops, c):
    r, _ = run_and_judge(ops, c)
    assert r["can_fuse_sc"] == 1, "igemm_can_fuse_shortcut said no to a launch that ran"


@pytest.mark.parametrize("c,word", IM.SHORTCUT_REFUSED, ids=ids(IM.SHORTCUT_REFUSED))
def test_shortcut_fold_refused(ops, c, word):
    r = refused(ops, c, word)
    assert r["can_fuse_sc"] == 0, "igemm_can_fuse_shortcut said yes to a launch that is refused"


# ------------------------------------------------------------------------------------------------------------------------------
# epilogue forms
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", IM.EPILOGUE, ids=ids(IM.EPILOGUE))
def test_epilogue_forms(ops, c):
    run_and_judge(ops, c)


@pytest.mark.parametrize("c", IM.SLAB, ids=ids(IM.SLAB))
def test_plain_slab_pass(ops, c):
    run_and_judge(ops, c, twice=True)


def _agree(ops, na, nb):
    a, b = IM.BY_NAME[na], IM.BY_NAME[nb]
    ga, gb = result(ops, a, launch(ops, a)).double().cpu(), result(ops, b, launch(ops, b)).double().cpu()
    ra = IM.reference(a)
    assert torch.equal(ra["want"], IM.reference(b)["want"]), "the pair does not state one problem"
    d = (ga - gb).abs()
    if a["out_f32"]:
        worst = float((d / (2 * ra["bound"])).max())
        print(f"igemm[{na} / {nb}]: worst difference / (2 x fp32 bound) {worst:.4f}")
        assert worst <= 1.0
    else:       # after the rounding: the two may round an element apart where their fp32 values straddle a tie -- one bf16 step of the element, rarely
        step = ra["want"].abs().clamp_min(2.0 ** -126) * 2.0 ** -7
        print(f"igemm[{na} / {nb}]: {float((d > 0).double().mean()):.5f} of the elements differ")
        assert bool((d <= step).all()) and float((d > 0).double().mean()) < 0.02


@pytest.mark.parametrize("na,nb", IM.EPILOGUE_PAIRS + IM.SLAB_PAIRS, ids=[a for a, _ in IM.EPILOGUE_PAIRS + IM.SLAB_PAIRS])
def test_vector_and_element_paths_agree(ops, na, nb):
    _agree(ops, na, nb)


# ------------------------------------------------------------------------------------------------------------------------------
# batched launches
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", IM.BATCHED, ids=ids(IM.BATCHED))
def test_batched_launches(ops, c):
    run_and_judge(ops, c)


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm fold
# ------------------------------------------------------------------------------------------------------------------------------
def _rowstat_check(c, r, got):
    M, N, Nout, K, HWo = IM.dims(c)
    table = r["rowstat"]
    assert bool((table[M:] == IM_SENTINEL).all()), "statistics rows >= M were written"
    bn = c["cfg"][1]
    v = torch.nn.functional.pad(got.double().cpu(), (0, (-N) % bn)).reshape(M, -1, bn)          # [M, slots, BN]: the launch's own bf16 output
    es, eq = IM.sums_errors(table[:M], v, 2, IM.rowstat_depth(c))
    print(f"igemm[{c['name']}]: rowstat error / bound: sum {es:.4f}, sum of squares {eq:.4f}")
    report(f"igemm_ops[{c['name']} rowstat]", sum_over_bound=es, squares_over_bound=eq)
    assert es <= 1.0 and eq <= 1.0


@pytest.mark.parametrize("c", IM.LN_PRODUCERS, ids=ids(IM.LN_PRODUCERS))
def test_layernorm_fold_producer(ops, c):
    r, got = run_and_judge(ops, c)
    _rowstat_check(c, r, got)


@pytest.mark.parametrize("c", IM.LN_CONSUMERS, ids=ids(IM.LN_CONSUMERS))
def test_layernorm_fold_consumer(ops, c):
    run_and_judge(ops, c)


def test_layernorm_fold_producer_feeds_consumer(ops):
    """as transformer() chains them: launch 1 leaves h (bf16) and its row statistics, launch 2 reads both.  The reference of launch 2 is
    fp64 on the h that launch 1 really returned -- the one bf16 rounding in between."""
    p = IM.BY_NAME["rowstat 64 wide tiles"]
    r1 = launch(ops, p)
    h = result(ops, p, r1)
    judge(p, h)
    M, N = h.shape
    c = IM.case("ln chained consumer", "general", cfg=(64, 64, 1), W=M, C0=N + (-N) % 64, N=136, ln={"slots": p["rowstat"]}, out_f32=False)
    i = IM.inputs(c)
    x = torch.zeros(M, c["C0"])
    x[:, :N] = h.float().cpu()                       # K is walked in 64-channel steps: the rows are padded with zeros, which the statistics do not see
    # LayerNorm over the N real channels: the producer's table and ln_invC = 1 / N state that
    xr = h.double().cpu()
    wfull = i["w4"][0].reshape(c["N"], -1).double()
    want = torch.nn.functional.layer_norm(xr, (N,), i["gamma"].double()[:N], i["beta"].double()[:N], float(torch.tensor(IM.LN_EPS, dtype=torch.float32))) @ wfull[:, :N].T + i["bias"].double()
    wf = (wfull[:, :N].float() * i["gamma"][:N].float()[None]).to(torch.bfloat16).double()
    cs, bf = wf.sum(1).float(), (i["bias"].double() + wfull[:, :N] @ i["beta"].double()[:N]).float()
    wpad = torch.zeros(c["N"], c["C0"])
    wpad[:, :N] = wf.float()
    r2 = ops.igemm(x.reshape(1, 1, M, -1).cuda(), wpad.cuda(), bias=bf.cuda(), ln_stats=r1["rowstat"][:M].contiguous(), ln_cs=cs.cuda(), ln_invC=1.0 / N,
                   ln_eps=IM.LN_EPS, out_f32=False)
    assert (r2["family"], r2["slab"], tuple(r2["cfg"])) == ("general", "none", (64, 64, 1))
    assert bool((r2["out"][M:] == IM_SENTINEL).all()), "rows >= M of the consumer's output were written"
    got = r2["out"][:M].double().cpu()
    S = r1["rowstat"][:M].double().cpu().sum(1)
    mu = (S[:, 0].float() * torch.tensor(1.0 / N)).double()
    var = (S[:, 1].float() * torch.tensor(1.0 / N) - mu.float() * mu.float()).clamp_min(0)
    rstd = (1.0 / torch.sqrt(var + torch.tensor(IM.LN_EPS))).double()
    model = IM._r(rstd[:, None] * (xr @ wf.T - mu[:, None] * cs.double()[None]) + bf.double()[None])
    e = IM.errors(c, got, want=want, model=model)
    print(f"igemm[producer -> consumer]: worst slab max {e['kernel_max']:.6f} (E_model {e['model_max']:.6f}), rms {e['kernel_rms']:.6f} (E_rms {e['model_rms']:.6f})")
    report("igemm_ops[ln producer -> consumer]", kernel_max=e["kernel_max"], model_max=e["model_max"], kernel_rms=e["kernel_rms"], model_rms=e["model_rms"])
    assert MODEL_FACTOR * e["model_max"] <= IM.MODEL_CEILING and not e["violations"], e


# ------------------------------------------------------------------------------------------------------------------------------
# GroupNorm statistics producer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", IM.COLSTAT, ids=ids(IM.COLSTAT))
def test_groupnorm_statistics_producer(ops, c):
    r, got = run_and_judge(ops, c)
    M, N, Nout, K, HWo = IM.dims(c)
    bm = c["cfg"][0]
    tiles = M // bm
    table = r["colstat"].reshape(-1)
    assert bool((table[tiles * N * 2:] == IM_SENTINEL).all()), "statistics tiles >= M / BM were written"
    table = table[:tiles * N * 2].reshape(tiles, N, 2)
    v = got.double().cpu().reshape(tiles, bm, N)
    es, eq = IM.sums_errors(table, v, 1, IM.colstat_depth(c))
    print(f"igemm[{c['name']}]: colstat error / bound: sum {es:.4f}, sum of squares {eq:.4f}")
    report(f"igemm_ops[{c['name']} colstat]", sum_over_bound=es, squares_over_bound=eq)
    assert es <= 1.0 and eq <= 1.0


@pytest.mark.parametrize("c,word", IM.COLSTAT_REFUSED, ids=ids(IM.COLSTAT_REFUSED))
def test_groupnorm_statistics_producer_refused(ops, c, word):
    refused(ops, c, word)


# ------------------------------------------------------------------------------------------------------------------------------
# slab sum + GroupNorm
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain(ops, name):
    c = IM.BY_NAME[name]
    return launch(ops, c, no_gn=True)


@pytest.mark.parametrize("c", IM.SLAB_GN, ids=ids(IM.SLAB_GN))
def test_slab_sum_with_groupnorm(ops, c):
    M, N, Nout, K, HWo = IM.dims(c)
    i = IM.inputs(c)
    plain = _plain(ops, c["name"])
    assert (plain["family"], plain["slab"], plain["gn_fused"]) == (c["family"], "plain", 0)
    keep = launch(ops, c, keep_out=1)
    act = result(ops, c, keep)
    assert keep["gn_fused"] == 1
    assert torch.equal(keep["out"], plain["out"]), "gn_keep_out: `out` differs from the plain slab pass"
    judge(c, act)
    drop = launch(ops, c, keep_out=0)
    assert drop["gn_fused"] == 1 and (drop["family"], drop["slab"]) == (c["family"], "gn")
    assert bool((drop["out"] == ops.IGEMM_SENTINEL).all()), "`out` was written without gn_keep_out"
    assert torch.equal(drop["gn_y"], keep["gn_y"]) and torch.equal(launch(ops, c, keep_out=1)["gn_y"], keep["gn_y"])
    # gn_y against the GroupNorm of the activation the launch itself rounded, per (image, group)
    g = c["gn"]["groups"]
    x = act.double().cpu().reshape(c["images"], HWo, N).transpose(1, 2)
    want = groupnorm_fp64(x, None, g, i["gn_gamma"], i["gn_beta"], IM.GN_EPS, bool(c["gn"].get("silu")))
    model = IM.gn_model(c, act.cpu()).reshape(c["images"], HWo, N).transpose(1, 2)
    got = keep["gn_y"].double().cpu().reshape(c["images"], HWo, N).transpose(1, 2)
    em, er = (float(v.max()) for v in slab_errors(gn_slabs(model, g), gn_slabs(want, g), gn_slabs(model, g)))
    km, kr = (float(v.max()) for v in slab_errors(gn_slabs(got, g), gn_slabs(want, g), gn_slabs(model, g)))
    print(f"igemm[{c['name']}] gn_y: worst slab max {km:.6f} (E_model {em:.6f}), rms {kr:.6f} (E_rms {er:.6f})")
    report(f"igemm_ops[{c['name']} gn_y]", kernel_max=km, model_max=em, kernel_rms=kr, model_rms=er)
    assert MODEL_FACTOR * em <= IM.MODEL_CEILING and km <= MODEL_FACTOR * em and kr <= MODEL_FACTOR * er
    # ... and against the separate path: the plain slab pass, then the GroupNorm kernels
    sep = ops.group_norm(act.reshape(c["images"], HWo, N).transpose(1, 2).contiguous(), g, i["gn_gamma"].cuda(), i["gn_beta"].cuda(), eps=IM.GN_EPS,
                         silu=bool(c["gn"].get("silu")))
    d = (sep.double().cpu() - got).abs()
    assert float(d.max()) <= float(want.abs().max()) * 2.0 ** -7 and float((d > 0).double().mean()) < 0.02, (float(d.max()), float((d > 0).double().mean()))


@pytest.mark.parametrize("c", IM.SLAB_GN_DECLINED, ids=ids(IM.SLAB_GN_DECLINED))
def test_slab_sum_with_groupnorm_declined(ops, c):
    r = launch(ops, c, keep_out=0)
    got = result(ops, c, r)                          # slab == "plain": the pass declined
    assert r["gn_fused"] == 0 and bool((r["gn_y"] == ops.IGEMM_SENTINEL).all())
    judge(c, got)


# ------------------------------------------------------------------------------------------------------------------------------
# per-image weights
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", IM.WPI, ids=ids(IM.WPI))
def test_per_image_weights(ops, c):
    run_and_judge(ops, c)


@pytest.mark.parametrize("c,word", IM.WPI_REFUSED, ids=ids(IM.WPI_REFUSED))
def test_per_image_weights_refused(ops, c, word):
    refused(ops, c, word)


# ------------------------------------------------------------------------------------------------------------------------------
# forms on which the epilogue's paths disagree: refused by the launcher
# ------------------------------------------------------------------------------------------------------------------------------
def _refusal_case(name, **kw):
    return IM.case(name, "none", W=200, C0=128, N=256, out_f32=False, **kw)


def test_geglu_without_bias_is_refused(ops):
    """both epilogue paths would read bias + Nout from a null pointer: the launcher says no, nothing runs"""
    refused(ops, _refusal_case("refused: geglu without bias", geglu=True, bias_mode=0), "geglu needs a per-column bias")
    c = _refusal_case("refused: geglu through ops.linear")
    i = IM.inputs(c)
    from agenda_amd._lib import AgendaHipError
    with pytest.raises(AgendaHipError, match="geglu needs a per-column bias"):
        ops.linear(i["x0"].reshape(200, 128).cuda(), i["w4"][0].reshape(256, 128).cuda(), None, geglu=True)


def test_geglu_with_rowadd_or_row_bias_is_refused(ops):
    refused(ops, _refusal_case("refused: geglu with rowadd", geglu=True, rowadd=True), "geglu takes no rowadd")
    c = _refusal_case("refused: geglu with a row bias", geglu=True)
    refused(ops, c, "geglu needs a per-column bias", bias_mode=2)


def test_layernorm_fold_with_alpha_or_row_bias_is_refused(ops):
    refused(ops, _refusal_case("refused: ln with alpha", ln={"slots": 2}, alpha=0.5), "LayerNorm fold needs alpha == 1")
    refused(ops, _refusal_case("refused: ln with a row bias", ln={"slots": 2}), "LayerNorm fold takes no per-row bias", bias_mode=2)


@pytest.mark.parametrize("what", ["rowadd address", "rowadd pitch", "bias address", "gamma address", "beta address"])
def test_fused_groupnorm_pass_falls_back_on_unaligned_operands(ops, what):
    """the fused pass reads bias / rowadd / gamma / beta as 16-byte quads: operands not aligned for that take the plain slab pass
    (`*gn_fused` stays 0) and `out` is the plain pass's, bit for bit"""
    c = IM.BY_NAME["gn 640 quads all forms"]
    M, N, Nout, K, HWo = IM.dims(c)
    t, kw = IM.launch_args(c)

    def off(v):                                      # the same values one float (4 bytes) into a fresh buffer
        b = torch.zeros(v.numel() + 1, device="cuda")
        b[1:] = v.reshape(-1).cuda()
        return b[1:].view(v.shape)

    dev = {k: (None if v is None else v.cuda()) for k, v in t.items()}
    gn = dict(c["gn"], gamma=dev.pop("gn_gamma"), beta=dev.pop("gn_beta"), eps=IM.GN_EPS, keep_out=1)
    if what == "rowadd address":
        dev["rowadd"] = off(t["rowadd"])
    elif what == "rowadd pitch":
        wide = torch.zeros(c["images"], N + 2, device="cuda")
        wide[:, :N] = dev["rowadd"]
        dev["rowadd"], kw["rowadd_ld"] = wide, N + 2
    elif what == "bias address":
        dev["bias"] = off(t["bias"])
    elif what == "gamma address":
        gn["gamma"] = off(t["gn_gamma"])
    else:
        gn["beta"] = off(t["gn_beta"])
    r = ops.igemm(dev.pop("src0"), dev.pop("w"), gn=gn, **dev, **kw)
    assert (r["family"], r["slab"], r["gn_fused"]) == (c["family"], "plain", 0), (r["family"], r["slab"], r["gn_fused"])
    assert bool((r["gn_y"] == ops.IGEMM_SENTINEL).all())
    assert torch.equal(r["out"], _plain(ops, c["name"])["out"])

"""Non-square outputs without a GPU: the rectangular DAAM restatement against the oracle's recorder on square maps, the size rule,
and the safety checker's resize + center-crop geometry against transformers' CLIP image processor."""
import numpy as np
import pytest
import torch

from _aspect_restated import AspectDaamRecorder, clip_resize_crop_geometry, inpaint_mask_latents


def _feed(rec, lh, lw, heads=2, T=77, b=2, seed=0):
    """Softmax-like maps of every UNet level of an SD-shaped walk (mid block included: both recorders must skip it)."""
    g = torch.Generator().manual_seed(seed)
    for lvl, layer in ((0, "down_blocks.0.attentions.0"), (1, "down_blocks.1.attentions.0"), (2, "up_blocks.1.attentions.2"),
                       (3, "mid_block.attentions.0"), (0, "up_blocks.3.attentions.1")):
        n = (lh >> lvl) * (lw >> lvl)
        p = torch.rand(2 * b * heads, n, T, generator=g).softmax(-1)
        rec(p, heads, layer)


@pytest.mark.parametrize("side", [16, 24, 64])
def test_rectangular_restatement_is_the_oracle_recorder_on_square_maps(side):
    from oracle import sd_oracle as O
    a, b = O.DaamRecorder(side * side, 77), AspectDaamRecorder((side, side), 77)
    _feed(a, side, side)
    _feed(b, side, side)
    assert a.acc.keys() == b.acc.keys()
    assert torch.equal(a.compute_global_heat_map(10), b.compute_global_heat_map(10))


@pytest.mark.parametrize("lh,lw", [(64, 96), (96, 64), (16, 24)])
def test_rectangular_restatement_shapes(lh, lw):
    rec = AspectDaamRecorder((lh, lw), 77)
    _feed(rec, lh, lw)
    assert {k[0] for k in rec.acc} == {1, 2, 4}                   # f = 8 (and the mid block) are not recorded
    for (f, _, _), m in rec.acc.items():
        assert m.shape == (2, 77, lh // f, lw // f)
    g = rec.compute_global_heat_map(5)
    assert g.shape == (2, 5, lh, lw) and bool((g >= 0).all())


@pytest.mark.parametrize("h,w,ok", [(512, 512, True), (512, 768, True), (768, 512, True), (64, 1024, True), (128, 192, True),
                                    (512, 700, False), (500, 512, False), (0, 512, False), (512, -64, False), (96, 64, False)])
def test_size_rule(h, w, ok):
    from agenda_amd.pipeline import check_image_size
    if ok:
        check_image_size(h, w)
    else:
        with pytest.raises(ValueError) as ei:
            check_image_size(h, w)
        assert f"height={h}" in str(ei.value) and f"width={w}" in str(ei.value)


def test_mask_latents_take_every_eighth_pixel_per_axis():
    m = torch.rand(2, 64, 96, generator=torch.Generator().manual_seed(3))
    got = inpaint_mask_latents(m)
    assert got.shape == (2, 1, 8, 12)
    assert torch.equal(got[:, 0], (m[:, ::8, ::8] >= 0.5).float())


@pytest.mark.parametrize("h,w", [(512, 768), (768, 512), (512, 512), (640, 384)])
def test_safety_resize_and_crop_geometry_matches_clip_image_processor(h, w):
    from PIL import Image
    try:
        from transformers import CLIPImageProcessorPil as Proc
    except ImportError:
        from transformers import CLIPImageProcessor as Proc
    rng = np.random.default_rng(h * 7 + w)
    im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    kw = dict(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, resample=3, do_rescale=False, do_normalize=False)
    resized = Proc(do_center_crop=False, **kw)(images=[Image.fromarray(im)], return_tensors="np").pixel_values[0]
    cropped = Proc(do_center_crop=True, **kw)(images=[Image.fromarray(im)], return_tensors="np").pixel_values[0]
    rh, rw, top, left = clip_resize_crop_geometry(h, w, 224)
    assert resized.shape == (3, rh, rw)
    assert np.array_equal(cropped, resized[:, top:top + 224, left:left + 224])


def test_generation_cli_takes_height_width_and_one_or_two_image_sizes():
    from agenda_amd.generation import parse_args
    a = parse_args(["--height", "512", "--width", "768", "--image-size", "112", "168"])
    assert (a.height, a.width, a.image_size) == (512, 768, (112, 168))
    b = parse_args(["--image-size", "96"])
    assert (b.height, b.width, b.image_size) == (None, None, 96)          # square output, the reference's resize((S, S))
    for bad in (["--height", "500"], ["--width", "0"], ["--image-size", "1", "2", "3"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_save_outputs_writes_rectangular_pngs_on_the_host_path(tmp_path):
    from PIL import Image
    from agenda_amd.generation import save_outputs
    rng = np.random.default_rng(0)
    imgs = rng.integers(1, 256, (2, 64, 96, 3), dtype=np.uint8)
    hms = rng.random((2, 1, 8, 12)).astype(np.float32)
    save_outputs(str(tmp_path), [3, 4], imgs, hms, ["car"], (48, 72))
    assert Image.open(tmp_path / "images" / "3.png").size == (72, 48)
    assert Image.open(tmp_path / "daam_car_heatmaps" / "4.png").size == (72, 48)


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _gather_worker(rank, world, port, out_dir):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from agenda_amd.generation import gather_outputs, shard_seeds
    seeds = shard_seeds(6, rank, world)
    imgs = torch.stack([torch.full((4, 6, 3), s, dtype=torch.uint8) for s in seeds])
    hms = torch.stack([torch.full((2, 8, 12), float(s)) for s in seeds])
    s_, gi, gh = gather_outputs(imgs, hms, seeds=seeds, max_batch=3)
    np.save(os.path.join(out_dir, f"i{rank}.npy"), gi.numpy())
    np.save(os.path.join(out_dir, f"h{rank}.npy"), gh.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_gather_outputs_with_rectangular_images_and_heat_maps(tmp_path):
    import torch.multiprocessing as mp
    mp.start_processes(_gather_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    for r in range(2):
        gi, gh = np.load(tmp_path / f"i{r}.npy"), np.load(tmp_path / f"h{r}.npy")
        assert gi.shape == (6, 4, 6, 3) and gh.shape == (6, 2, 8, 12)
        assert [int(x) for x in gi[:, 0, 0, 0]] == list(range(6)) and [float(x) for x in gh[:, 0, 0, 0]] == list(range(6))

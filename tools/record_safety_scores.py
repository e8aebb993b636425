"""Records agd_safety_scores_hw of whatever build this tree holds, in the form of tests/golden/safety_scores_parent.npz: the tiny config with
a 3 + 17 concept safety checker (hidden 128, 2 layers, 2 heads, MLP 256, projection 64; synthetic weights, seed 21) on a rectangular batch
(2 images of 160 x 208, seed 31) and a square one (3 of 224 x 224, seed 32) -- the cosines as they come, and the preprocessed pixels as one
fp64 sum per image.

    python tools/record_safety_scores.py OUT.npz [--compare tests/golden/safety_scores_parent.npz]

The committed file was written by this script's body in a checkout of commit 6d8f2a9 ("Add T2I-Adapter conditioned txt2img with the features
added on device"), the last one whose safety entry ran its own vision path, built for gfx950 and run on one MI355X.  It uses nothing newer
than that commit, so the recording can be made again there; tests/test_ip_adapter_gpu.py compares the current build with it bit for bit."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"rect": (2, 160, 208, 31), "square": (3, 224, 224, 32)}


def images(n, h, w, seed):
    """Random uint8 images over a per-image colour ramp (tests/test_ip_adapter_gpu.py draws the same ones)."""
    rng = np.random.default_rng(seed)
    ry, rx = np.linspace(0, 1, h, dtype=np.float32), np.linspace(0, 1, w, dtype=np.float32)
    out = []
    for _ in range(n):
        base = rng.uniform(0, 255, 3) * ry[:, None, None] + rng.uniform(0, 255, 3) * rx[None, :, None] * (1 - ry[:, None, None])
        out.append(np.clip(base + rng.normal(0, 40, (h, w, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--compare", help="an earlier recording; exit status 1 unless every array is bit-identical")
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionPipeline, config, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("record_safety_scores: no GPU visible")
    cfg = config.tiny()
    cfg.safety = config.SafetyConfig(n_special=3, n_concepts=17, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                                     projection_dim=64)
    pipe = StableDiffusionPipeline(cfg, synthetic.make_unet_weights(cfg), synthetic.make_vae_weights(cfg), safety_sd=synthetic.make_safety_weights(cfg, 21),
                                   workspace_bytes=1 << 30)
    rec = {}
    for name, (n, h, w, seed) in CASES.items():
        cos, pix = pipe.safety_checker.scores(torch.from_numpy(images(n, h, w, seed)).cuda(), pixels=True)
        rec[name + "_cos"] = cos.cpu().numpy()
        rec[name + "_pix_sum"] = pix.double().sum(dim=(1, 2, 3)).cpu().numpy()
    pipe.engine.close()
    np.savez(args.out, **rec)
    if args.compare:
        old = np.load(args.compare)
        same = {k: bool(np.array_equal(old[k], v)) for k, v in rec.items()}
        print(same)
        if not all(same.values()) or set(old.files) != set(rec):
            raise SystemExit(1)


if __name__ == "__main__":
    main()

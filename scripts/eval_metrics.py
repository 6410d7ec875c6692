#!/usr/bin/env python3
"""PSNR and SSIM of a directory of rendered frames against a split's ground truth, on the device: the counterpart of the
reference's tools/eval_metrics.py.

    python scripts/eval_metrics.py --split_path <scene>/transforms_test.json --res_img_dir <results>

Reads `rgb_fine_{idx:03d}.png` for every frame of the split and the frame's ground-truth image next to the split file
(`<file_path>.png` for the synthetic scenes, `<file_path>` otherwise), blends RGBA on white, brings the ground truth to the
result's size with a LANCZOS resize as the reference does, stacks the frames on the device and prints
`Mean PSNR ... SSIM ... LPIPS n/a` (LPIPS needs the weights of a network this package does not carry).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_image(path, resize_wh=None):
    """(H, W, 3) float32 in [0, 1] (what torchvision's ToTensor gives, channels last), and (W, H)."""
    import numpy as np
    from PIL import Image
    img = Image.open(path)
    if resize_wh is not None:
        img = img.resize(resize_wh, Image.LANCZOS)
    a = np.asarray(img, dtype=np.float32) / np.float32(255.0)
    if a.ndim == 2:
        a = a[..., None]
    if a.shape[-1] == 4:      # RGBA: blend on white
        a = a[..., :3] * a[..., 3:] + (1 - a[..., 3:])
    return a, (a.shape[1], a.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--split_path", type=str, required=True)
    ap.add_argument("--res_img_dir", type=str, required=True)
    args = ap.parse_args()
    import numpy as np
    import torch
    from mirror_nerf_amd import metrics
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics.py computes on the GPU only")
    with open(args.split_path) as f:
        meta = json.load(f)
    root_dir = os.path.split(args.split_path)[0]
    groups = {}      # frames of one size go to the device as one stack
    for idx, frame in enumerate(meta["frames"]):
        res, res_wh = load_image(os.path.join(args.res_img_dir, f"rgb_fine_{idx:03d}.png"))
        file_path = f"{frame['file_path']}.png" if "mirror_syn_scene" in root_dir else frame["file_path"]
        gt, _ = load_image(os.path.join(root_dir, file_path), resize_wh=res_wh)
        groups.setdefault(res.shape, []).append((res, gt))
    psnr, ssim = [], []
    for pairs in groups.values():
        p = torch.from_numpy(np.stack([a for a, _ in pairs])).to("cuda:0")
        t = torch.from_numpy(np.stack([b for _, b in pairs])).to("cuda:0")
        a, b = metrics.frame_metrics(p, t)
        psnr.append(a.double())
        ssim.append(b.double())
    n = sum(len(v) for v in groups.values())
    if n == 0:
        raise SystemExit("the split has no frames")
    print("Mean PSNR {} SSIM {} LPIPS n/a".format(float(torch.cat(psnr).sum()) / n, float(torch.cat(ssim).sum()) / n))


if __name__ == "__main__":
    main()

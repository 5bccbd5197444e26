"""Image metrics of a rendered sequence against its test images: the reference's nerf/metrics.py (`two_folders`) with the numbers
computed on the device by libnerface_hip.so (nf_image_metrics: one launch per batch of frames) instead of skimage on the host.

    python -m nerf.metrics --gt_path data/test --images_path renders

L1, PSNR and SSIM are the reference's: np.mean(np.abs(.)), compare_psnr and compare_ssim(multichannel=True) of the float images
byte / 255 -- including that skimage's choice of the SSIM data range for float input, 2 (`ssim_data_range`; 1.0 gives the textbook
constants).  LPIPS is not computed: it needs the `lpips` package and its trained AlexNet weights, and this package ships neither.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from .ops import image_metrics

LPIPS_NOTE = "# LPIPS is not computed (it needs the lpips package and its AlexNet weights); L1 / PSNR / SSIM as nerf/metrics.py reports them\n"


def write_metrics_file(path: str, rows, path_gt: str, path_generated: str) -> dict:
    """metrics.txt in the reference's layout (per frame `name   L1:`, `PSNR:`, `SSIM:` and an empty line; a summary of the means),
    without its LPIPS lines.  rows: (file name, l1, psnr, ssim).  Returns {"frames", "mean_l1", "mean_psnr", "mean_ssim"}."""
    n = len(rows)
    means = {"frames": n}
    for k, key in enumerate(("mean_l1", "mean_psnr", "mean_ssim"), start=1):
        means[key] = float(sum(r[k] for r in rows) / (n if n > 0 else 1))
    with open(path, "w") as fo:
        fo.write(LPIPS_NOTE)
        for name, l1, psnr, ssim in rows:
            fo.write(name + "   L1:  \t%5f \n" % l1)
            fo.write(name + "   PSNR:\t%5f \n" % psnr)
            fo.write(name + "   SSIM:\t%5f \n\n" % ssim)
        fo.write(summary_text(means, path_gt, path_generated))
    return means


def summary_text(means: dict, path_gt: str, path_generated: str) -> str:
    return ("=" * 80 + "\n Summary \n folder 1: %s \n folder 2: %s \n" % (path_gt, path_generated) + "-" * 80
            + "\n mean L1:\t%5f" % means["mean_l1"] + "\n mean PSNR:\t%5f" % means["mean_psnr"] + "\n mean SSIM:\t%5f\n" % means["mean_ssim"])


def _frame_number(name: str) -> int:
    digits = "".join(filter(str.isdigit, name))
    if not digits:
        raise ValueError(f"two_folders: {name!r} has no number in its name; the folders are paired by the numbers in their file names")
    return int(digits)


def _is_png(name: str) -> bool:
    parts = name.split(".")                                    # the reference's rule: the FIRST extension is png
    return len(parts) > 1 and parts[1] == "png"


def _read_rgb_u8(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        arr = np.array(im)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"{path}: expected an 8-bit RGB image, got {arr.dtype} {arr.shape}")
    return arr


def _save_l2_image(gt: np.ndarray, gen: np.ndarray, path: str) -> None:
    """Per-pixel L2 distance of the float images through the jet colour map, scaled to its own range, at the native resolution."""
    from PIL import Image
    d = np.linalg.norm(gt.astype(np.float64) / 255 - gen.astype(np.float64) / 255, axis=2)
    t = (d - d.min()) / (d.max() - d.min() + 1e-12)
    rgb = np.stack([1.5 - np.abs(4 * t - 3), 1.5 - np.abs(4 * t - 2), 1.5 - np.abs(4 * t - 1)], axis=-1).clip(0, 1)
    Image.fromarray((rgb * 255).astype(np.uint8)).save(path)


def two_folders(path_gt, path_generated, save_l2: bool = False, ssim_data_range: float = 2.0, batch: int = 16, device=None):
    """Compare the i-th generated PNG with the i-th entry of the ground-truth folder, both sorted by the number in the file name
    (the generated folder's regular files whose first extension is png; every entry of the ground-truth folder), print the summary and
    write path_generated/metrics.txt.  Returns the means.  save_l2: also write path_generated/L2/%04d.png."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    names_gt = os.listdir(os.path.join(path_gt))
    names_gen = [f for f in os.listdir(path_generated)
                 if os.path.isfile(os.path.join(path_generated, f)) and _is_png(f)]
    names_gt.sort(key=_frame_number)
    names_gen.sort(key=_frame_number)
    if len(names_gen) > len(names_gt):
        raise ValueError(f"two_folders: {len(names_gen)} rendered frames in {path_generated} but only {len(names_gt)} entries in {path_gt}")
    print(f"{len(names_gt)} ground-truth entries in {path_gt}, {len(names_gen)} rendered frames in {path_generated}")
    if save_l2:
        os.makedirs(os.path.join(path_generated, "L2"), exist_ok=True)
    results, pend_gt, pend_gen = [], [], []                    # device results per batch; frames of one shape waiting for their launch

    def flush():
        if pend_gen:
            gen = torch.from_numpy(np.stack(pend_gen)).to(device, non_blocking=True)
            gt = torch.from_numpy(np.stack(pend_gt)).to(device, non_blocking=True)
            m = image_metrics(gen, gt, ssim_data_range=ssim_data_range)
            results.append(torch.stack([m["l1"], m["psnr"], m["ssim"]], dim=1))
            pend_gt.clear()
            pend_gen.clear()

    for i, name in enumerate(names_gen):
        im_real = _read_rgb_u8(os.path.join(path_gt, names_gt[i]))
        im_generated = _read_rgb_u8(os.path.join(path_generated, name))
        assert im_real.shape == im_generated.shape
        if save_l2:
            _save_l2_image(im_real, im_generated, os.path.join(path_generated, "L2", "%04d.png" % i))
        if pend_gen and (pend_gen[0].shape != im_generated.shape or len(pend_gen) >= batch):
            flush()
        pend_gt.append(im_real)
        pend_gen.append(im_generated)
    flush()
    values = torch.cat(results).cpu().tolist() if results else []          # the one read-back
    rows = [(name, v[0], v[1], v[2]) for name, v in zip(names_gen, values)]
    means = write_metrics_file(os.path.join(path_generated, "metrics.txt"), rows, path_gt, path_generated)
    print(summary_text(means, path_gt, path_generated))
    return means


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="L1 / PSNR / SSIM of a folder of rendered frames against a folder of test images")
    parser.add_argument("--gt_path", type=str, default="", help="folder of the test images, one per frame")
    parser.add_argument("--images_path", type=str, default="", help="folder of the rendered PNGs; metrics.txt is written here")
    parser.add_argument("--save-l2", action="store_true", help="also write the per-pixel L2 images to <images_path>/L2")
    parser.add_argument("--ssim-data-range", type=float, default=2.0, help="2.0 = as the reference computes it; 1.0 = textbook")
    opt = parser.parse_args()
    two_folders(opt.gt_path, opt.images_path, save_l2=opt.save_l2, ssim_data_range=opt.ssim_data_range)

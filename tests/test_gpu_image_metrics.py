"""GPU: nf_image_metrics (L1, MSE, PSNR, SSIM of uint8 frames on the device) against the float64 restatement of
tests/metrics_ref.py at every size edge of its 32 x 32-origin tiles, through nerf.image_metrics, the eval launcher's --metrics and
nerf.metrics.two_folders."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILE, HALO = 32, 6                    # nfm::TILE, nfm::HALO of csrc/nf_metrics.hip: one tile covers TILE + HALO = 38 pixels
EDGE = TILE + HALO
SMALL = [(7, 7), (7, 8), (8, 7), (EDGE - 1, EDGE), (EDGE, EDGE - 1), (EDGE, EDGE), (EDGE + 1, EDGE), (EDGE, EDGE + 1), (33, 65), (64, 64)]
LARGE = [(1030, 1019), (512, 512)]
ULP4 = lambda want: 4 * np.spacing(abs(np.float64(want)))
SSIM_GATE = 1e-12


def _pixel_spots(h, w):
    """The four corners, and the two sides of a tile seam (the last column a tile reads beyond its origins / the first origin of
    the next tile), clipped to the image."""
    return [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (min(TILE - 1, h - 1), min(EDGE - 1, w - 1)), (min(TILE, h - 1), min(TILE, w - 1))]


@functools.lru_cache(maxsize=None)
def _batch(h, w, full):
    """Image pairs of one shape and their restatement for both data ranges, computed once per session."""
    pairs = [R.random_pair(h, w, 11), R.gradient_pair(h, w, 12)]
    if full:
        pairs += [R.identical_pair(h, w, 13), R.black_white_pair(h, w)]
        pairs += [R.one_pixel_pair(h, w, 14, y, x, channel=k % 3) for k, (y, x) in enumerate(_pixel_spots(h, w))]
    else:                                                          # many tiles: +inf PSNR / SSIM 1 and the extremes through the reduction too
        y, x = _pixel_spots(h, w)[-1]
        pairs += [R.one_pixel_pair(h, w, 14, y, x), R.identical_pair(h, w, 13), R.black_white_pair(h, w)]
    ref = {}
    for k, (a, b) in enumerate(pairs):
        stats = R.window_stats(a, b)
        for data_range in (1.0, 2.0):
            ref[k, data_range] = R.metrics_int(a, b, data_range, stats)
    return pairs, ref


def _run(nerf, gpu, pairs, data_range):
    a = torch.from_numpy(np.stack([p[0] for p in pairs])).to(gpu)
    b = torch.from_numpy(np.stack([p[1] for p in pairs])).to(gpu)
    return {k: v.cpu().numpy() for k, v in nerf.image_metrics(a, b, ssim_data_range=data_range).items()}


def _check(got, ref, index, data_range, tag):
    worst = 0.0
    for k in index:
        want = ref[k, data_range]
        row = {name: got[name][k] for name in got}
        print(tag, "image", k, "R", data_range, {n: (float(row[n]), float(want[n])) for n in ("l1", "mse", "psnr", "ssim")},
              "ssim diff", abs(float(row["ssim"]) - float(want["ssim"])))
        assert int(row["abs_sum"]) == want["abs_sum"] and int(row["sq_sum"]) == want["sq_sum"], (tag, k, row, want)
        assert abs(row["l1"] - want["l1"]) <= ULP4(want["l1"]) and abs(row["mse"] - want["mse"]) <= ULP4(want["mse"]), (tag, k, row, want)
        if np.isinf(want["psnr"]):
            assert row["psnr"] == np.inf and want["sq_sum"] == 0, (tag, k, row)
        else:
            assert abs(row["psnr"] - want["psnr"]) <= ULP4(want["psnr"]), (tag, k, row["psnr"], want["psnr"])
        d = abs(float(row["ssim"]) - float(want["ssim"]))
        assert d <= SSIM_GATE, (tag, k, data_range, row["ssim"], want["ssim"])
        worst = max(worst, d)
    return worst


@pytest.mark.parametrize("h,w", SMALL + LARGE)
def test_values_against_the_restatement(hip_lib, gpu, h, w):
    """Every content in ONE launch (N = 10 at the small shapes, 5 at the large ones, all images different), both data ranges: the
    integers exactly, l1 / mse / finite psnr within 4 ulps, psnr = +inf for identical images, ssim within 1e-12."""
    import nerf
    pairs, ref = _batch(h, w, (h, w) in SMALL)
    worst = 0.0
    for data_range in (2.0, 1.0):
        got = _run(nerf, gpu, pairs, data_range)
        assert all(v.shape == (len(pairs),) for v in got.values())
        assert got["l1"].dtype == np.float64 and got["ssim"].dtype == np.float64 and got["abs_sum"].dtype == np.int64
        worst = max(worst, _check(got, ref, range(len(pairs)), data_range, f"{h}x{w}"))
    print(f"{h}x{w}: worst |ssim - restatement| {worst:.3e} (gate {SSIM_GATE})")
    if (h, w) in LARGE:
        assert ref[3, 2.0]["ssim"] == 1.0 and np.isinf(ref[3, 2.0]["psnr"]) and ref[4, 2.0]["mse"] == 1.0
    if (h, w) == (64, 64):                                         # the contents are what they are meant to be
        assert ref[2, 2.0]["ssim"] == 1.0 and 0.3 < ref[1, 1.0]["ssim"] < ref[1, 2.0]["ssim"] < 0.95 and ref[0, 2.0]["ssim"] < 0.1


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", [(7, 7), (EDGE + 1, EDGE + 1), (33, 65), (512, 512)])
def test_batch_sizes_one_and_three(hip_lib, gpu, h, w, n):
    import nerf
    pairs, ref = _batch(h, w, (h, w) in SMALL)
    got = _run(nerf, gpu, pairs[:n], 2.0)
    _check(got, ref, range(n), 2.0, f"{h}x{w} n={n}")
    if n == 1:                                                     # a single (H, W, 3) image: 0-d results, the same bits
        one = nerf.image_metrics(torch.from_numpy(pairs[0][0]).to(gpu), torch.from_numpy(pairs[0][1]).to(gpu))
        assert all(v.dim() == 0 for v in one.values())
        assert all(one[k].cpu().numpy().tobytes() == got[k][0].tobytes() for k in got)


def test_empty_batch_returns_empty_tensors(hip_lib, gpu):
    import nerf
    e = torch.empty((0, 16, 16, 3), dtype=torch.uint8, device=gpu)
    out = nerf.image_metrics(e, e)
    assert set(out) == {"l1", "mse", "psnr", "ssim", "abs_sum", "sq_sum"} and all(v.shape == (0,) and v.is_cuda for v in out.values())
    assert out["ssim"].dtype == torch.float64 and out["sq_sum"].dtype == torch.int64


@pytest.mark.parametrize("h,w", [(EDGE + 1, EDGE + 1), (512, 512)])
def test_two_launches_are_bit_identical_and_buffers_may_hold_anything(hip_lib, gpu, h, w):
    """Run to run the same bits (fixed-order reduction); and the same bits again from the C entry point with the workspace and
    both outputs pre-filled with 0xFF bytes: nothing is read before it is written, the tickets are reset per call."""
    import nerf
    from nerf import _hip as H
    pairs, _ = _batch(h, w, (h, w) in SMALL)
    pairs = pairs[:3]
    a = torch.from_numpy(np.stack([p[0] for p in pairs])).to(gpu)
    b = torch.from_numpy(np.stack([p[1] for p in pairs])).to(gpu)
    first, second = nerf.image_metrics(a, b), nerf.image_metrics(a, b)
    for k in first:
        assert first[k].cpu().numpy().tobytes() == second[k].cpu().numpy().tobytes(), k
    n = len(pairs)
    need = hip_lib.nf_image_metrics_workspace_bytes(n, h, w)
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=gpu)
    of = torch.full((n * 4 * 8 + 64,), 0xFF, dtype=torch.uint8, device=gpu)
    oi = torch.full((n * 2 * 8 + 64,), 0xFF, dtype=torch.uint8, device=gpu)
    H.check(hip_lib.nf_image_metrics(H.ptr(a), H.ptr(b), n, h, w, 2.0, H.ptr(ws), need, H.ptr(of), H.ptr(oi), H.stream_ptr(gpu)), "nf_image_metrics")
    torch.cuda.synchronize()
    got_f = of[:n * 32].cpu().numpy().view(np.float64).reshape(n, 4)
    got_i = oi[:n * 16].cpu().numpy().view(np.int64).reshape(n, 2)
    for k, name in enumerate(("l1", "mse", "psnr", "ssim")):
        assert got_f[:, k].tobytes() == first[name].cpu().numpy().tobytes(), name
    assert got_i[:, 0].tobytes() == first["abs_sum"].cpu().numpy().tobytes() and got_i[:, 1].tobytes() == first["sq_sum"].cpu().numpy().tobytes()
    for buf, used in ((ws, need), (of, n * 32), (oi, n * 16)):     # nothing written past the stated sizes
        assert bool((buf[used:] == 0xFF).all())


def test_errors_are_raised_before_any_launch(hip_lib, gpu):
    import nerf
    u8 = torch.zeros((9, 9, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises(TypeError, match="quantize_image"):
        nerf.image_metrics(u8.float(), u8)
    with pytest.raises(TypeError, match="quantize_image"):
        nerf.image_metrics(u8, u8.to(torch.int32))
    with pytest.raises(ValueError):
        nerf.image_metrics(u8, torch.zeros((9, 10, 3), dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError):
        nerf.image_metrics(u8[:6], u8[:6])
    with pytest.raises(ValueError):
        nerf.image_metrics(u8[:, :6], u8[:, :6])
    with pytest.raises(ValueError):
        nerf.image_metrics(u8[..., :2], u8[..., :2])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nerf.image_metrics(u8.cpu(), u8)
    q = nerf.quantize_image((torch.arange(256, device=gpu, dtype=torch.float64) / 255).float())
    assert q.dtype == torch.uint8 and q.cpu().tolist() == list(range(256))


def _parse_metrics_file(path):
    per_frame, means = {}, {}
    for line in open(path):
        parts = line.split()
        if len(parts) == 3 and parts[0].endswith(".png"):
            per_frame.setdefault(parts[0], {})[parts[1].rstrip(":")] = float(parts[2])
        elif len(parts) == 3 and parts[0] == "mean":
            means[parts[1].rstrip(":")] = float(parts[2])
    return per_frame, means


def test_launcher_metrics_and_two_folders(hip_lib, gpu, tmp_path):
    """eval_sharded --metrics on the synthetic dataset (3 frames of 32 x 32, an untrained model): metrics.txt and last_stats equal
    the restatement applied to the PNGs the run wrote and the loader's test images; without the flag no metrics.txt and the same PNG
    bytes; two_folders on the same folders gives the same means."""
    import yaml
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))
    import make_synthetic_dataset as MS
    import nerf
    from launch import common as CM
    from launch import eval_sharded
    from nerf import metrics as MET
    from PIL import Image
    base = str(tmp_path)
    data = MS.write(os.path.join(base, "data"))
    cfg_path = os.path.join(base, "config.yml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(MS.config(data, os.path.join(base, "logs")), f)
    torch.manual_seed(7)
    model_c, model_f = CM.build_models(CM.load_config(cfg_path), gpu)
    ck_path = os.path.join(base, "untrained.ckpt")
    torch.save({"model_coarse_state_dict": model_c.state_dict(), "model_fine_state_dict": model_f.state_dict()}, ck_path)
    out, plain = os.path.join(base, "render_metrics"), os.path.join(base, "render_plain")
    torch.manual_seed(3)                                              # validation perturbs the depths: the same draws in both runs
    assert eval_sharded.main(["--config", cfg_path, "--checkpoint", ck_path, "--savedir", out, "--metrics"]) == [0, 1, 2]
    stats = eval_sharded.main.last_stats
    torch.manual_seed(3)
    assert eval_sharded.main(["--config", cfg_path, "--checkpoint", ck_path, "--savedir", plain]) == [0, 1, 2]
    assert "metrics" not in eval_sharded.main.last_stats and not os.path.exists(os.path.join(plain, "metrics.txt"))
    names = [f"{i:04d}.png" for i in range(3)]
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(plain, name), "rb").read(), name
    images = nerf.load_flame_data(data, half_res=False, testskip=1, test=True)[0].numpy()
    want = []
    for i, name in enumerate(names):
        frame = np.asarray(Image.open(os.path.join(out, name)))
        target = np.rint(np.clip(images[i][..., :3], 0, 1) * np.float32(255.0)).astype(np.uint8)
        assert np.array_equal(target, np.asarray(Image.open(os.path.join(data, "test", f"f_{i:04d}.png")))[..., :3])
        want.append(R.metrics_int(frame, target, 2.0))
    per_frame, means = _parse_metrics_file(os.path.join(out, "metrics.txt"))
    print("launcher metrics:", stats["metrics"], "metrics_s", stats["metrics_s"], "restatement:", want)
    assert sorted(per_frame) == names
    half_digit = 5.0e-7 + 1e-12                                       # the file holds six decimals
    for name, m in zip(names, want):
        assert abs(per_frame[name]["L1"] - m["l1"]) <= half_digit and abs(per_frame[name]["PSNR"] - m["psnr"]) <= half_digit
        assert abs(per_frame[name]["SSIM"] - m["ssim"]) <= half_digit
    mean = lambda key: sum(float(m[key]) for m in want) / 3
    assert stats["metrics"]["frames"] == 3 and stats["metrics_s"] > 0
    assert abs(stats["metrics"]["mean_l1"] - mean("l1")) <= ULP4(mean("l1")) and abs(stats["metrics"]["mean_psnr"] - mean("psnr")) <= ULP4(mean("psnr"))
    assert abs(stats["metrics"]["mean_ssim"] - mean("ssim")) <= SSIM_GATE
    assert abs(means["L1"] - mean("l1")) <= half_digit and abs(means["PSNR"] - mean("psnr")) <= half_digit and abs(means["SSIM"] - mean("ssim")) <= half_digit
    # the same folders through two_folders: one launch for the three frames, the same bits per frame, so the same means
    got = MET.two_folders(os.path.join(data, "test"), out)
    assert got == stats["metrics"], (got, stats["metrics"])
    assert not os.path.exists(os.path.join(out, "L2"))
    per_frame2, means2 = _parse_metrics_file(os.path.join(out, "metrics.txt"))
    assert per_frame2 == per_frame and means2 == means

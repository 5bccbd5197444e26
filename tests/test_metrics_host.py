"""CPU: the float64 restatement of the image metrics (tests/metrics_ref.py) against itself and against closed forms, the host side
of nf_image_metrics (argument checks before any launch) and the Python surface (nerf.image_metrics, nerf.quantize_image,
nerf.metrics.two_folders)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

SHAPES = [(7, 7), (7, 8), (8, 7), (33, 65), (64, 64), (37, 39)]


def _cases(h, w):
    return {"random": R.random_pair(h, w, 1), "gradient": R.gradient_pair(h, w, 2), "identical": R.identical_pair(h, w, 3),
            "black_white": R.black_white_pair(h, w), "pixel_first": R.one_pixel_pair(h, w, 4, 0, 0),
            "pixel_last": R.one_pixel_pair(h, w, 4, h - 1, w - 1)}


@pytest.mark.parametrize("h,w", SHAPES)
def test_integer_form_agrees_with_uniform_filter_form(h, w):
    """The integer-exact SSIM against the one built on scipy.ndimage.uniform_filter (skimage's own construction).  Measured over these
    shapes, contents and both data ranges: worst |difference| 6.4e-15 (float64 cancellation in uxx - ux ux of the filtered form);
    the gate is 10 x that."""
    for name, (a, b) in _cases(h, w).items():
        for data_range in (1.0, 2.0):
            exact = R.metrics_int(a, b, data_range)["ssim"]
            filt = R.ssim_uniform_filter(a, b, data_range)
            print(h, w, name, data_range, exact, abs(exact - filt))
            assert abs(exact - filt) <= 6.4e-14, (name, data_range, exact, filt)
            sk = R.ssim_skimage(a, b, data_range)                  # only where skimage is installed
            if sk is not None:
                assert abs(exact - sk) <= 6.4e-14, (name, data_range, exact, sk)


def test_gradient_case_is_mid_range_and_data_range_matters():
    a, b = R.gradient_pair(64, 64, 2)
    s2, s1 = R.metrics_int(a, b, 2.0)["ssim"], R.metrics_int(a, b, 1.0)["ssim"]
    assert 0.3 < s1 < s2 < 0.95                                    # larger constants pull S towards 1


@pytest.mark.parametrize("h,w", [(7, 7), (33, 65)])
def test_closed_forms(h, w):
    a, b = R.identical_pair(h, w, 5)
    m = R.metrics_int(a, b)
    assert m["ssim"] == 1.0 and m["l1"] == 0.0 and m["mse"] == 0.0 and m["psnr"] == np.inf and m["abs_sum"] == 0 and m["sq_sum"] == 0
    # two constant images: every variance and covariance is 0, S = (2 a b + C1) / (a^2 + b^2 + C1) at every pixel
    for va, vb in ((0, 255), (10, 200), (255, 255), (0, 0), (77, 78)):
        for data_range in (1.0, 2.0):
            ca, cb = np.full((h, w, 3), va, np.uint8), np.full((h, w, 3), vb, np.uint8)
            fa, fb, c1 = va / 255.0, vb / 255.0, (0.01 * data_range) ** 2
            want = (2 * fa * fb + c1) / (fa * fa + fb * fb + c1)
            got = R.metrics_int(ca, cb, data_range)
            assert abs(got["ssim"] - want) <= 4 * np.finfo(np.float64).eps, (va, vb, got["ssim"], want)
            assert got["abs_sum"] == abs(va - vb) * h * w * 3 and got["sq_sum"] == (va - vb) ** 2 * h * w * 3
    # one byte of one channel differs by 37 (or wraps: 256 - 37)
    pa, pb = R.one_pixel_pair(h, w, 4, h - 1, 0, channel=2, delta=37)
    d = abs(int(pa[h - 1, 0, 2]) - int(pb[h - 1, 0, 2]))
    assert d in (37, 219)
    m = R.metrics_int(pa, pb)
    assert m["abs_sum"] == d and m["sq_sum"] == d * d
    assert m["l1"] == d / (255.0 * h * w * 3) and m["mse"] == d * d / (65025.0 * h * w * 3)
    assert abs(m["psnr"] - 10 * np.log10(65025.0 * h * w * 3 / (d * d))) < 1e-12


def test_quantize_image_round_trips_every_byte():
    import nerf
    k = np.arange(256)
    as_loaded = (k / 255.0).astype(np.float32)                     # a test image as the loaders hold it (load_flame.py)
    want = np.clip(np.rint(np.clip(as_loaded, 0, 1) * np.float32(255.0)), 0, 255).astype(np.uint8)
    assert np.array_equal(want, k)
    got = nerf.quantize_image(torch.from_numpy(as_loaded))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), k)
    assert nerf.quantize_image(torch.tensor([-0.5, 1.5, 0.5 / 255 + 1e-4])).tolist() == [0, 255, 1]


def test_library_exports_and_refuses_bad_arguments_without_a_launch(hip_lib):
    assert hasattr(hip_lib, "nf_image_metrics") and hasattr(hip_lib, "nf_image_metrics_workspace_bytes")
    h, w, n = 16, 20, 2
    need = hip_lib.nf_image_metrics_workspace_bytes(n, h, w)
    assert need >= n * 4 + n * 3 * 8 and hip_lib.nf_image_metrics_workspace_bytes(3, 512, 512) > hip_lib.nf_image_metrics_workspace_bytes(1, 512, 512)
    a = np.zeros((n, h, w, 3), np.uint8)
    ws, of, oi = np.zeros(need, np.uint8), np.zeros((n, 4)), np.zeros((n, 2), np.int64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    call = lambda pa, pb, nn, hh, ww, pws, nws, pf, pi: hip_lib.nf_image_metrics(pa, pb, nn, hh, ww, 2.0, pws, nws, pf, pi, None)
    EINVAL = -22
    assert call(None, p(a), n, h, w, p(ws), need, p(of), p(oi)) == EINVAL
    assert call(p(a), None, n, h, w, p(ws), need, p(of), p(oi)) == EINVAL
    assert call(p(a), p(a), n, h, w, None, need, p(of), p(oi)) == EINVAL
    assert call(p(a), p(a), n, h, w, p(ws), need, None, p(oi)) == EINVAL
    assert call(p(a), p(a), n, h, w, p(ws), need, p(of), None) == EINVAL
    assert call(p(a), p(a), n, 6, w, p(ws), need, p(of), p(oi)) == EINVAL
    assert call(p(a), p(a), n, h, 6, p(ws), need, p(of), p(oi)) == EINVAL
    assert call(p(a), p(a), -1, h, w, p(ws), need, p(of), p(oi)) == EINVAL
    assert call(p(a), p(a), n, h, w, p(ws), need - 1, p(of), p(oi)) == EINVAL
    assert call(None, None, 0, h, w, None, 0, None, None) == 0           # n == 0: nothing to do, empty tensors have NULL pointers
    assert not of.any() and not oi.any() and not ws.any()


def test_python_surface():
    import nerf
    from nerf import metrics
    sig = inspect.signature(nerf.image_metrics)
    assert list(sig.parameters) == ["pred_u8", "target_u8", "ssim_data_range"] and sig.parameters["ssim_data_range"].default == 2.0
    assert list(inspect.signature(nerf.quantize_image).parameters) == ["x"]
    sig = inspect.signature(metrics.two_folders)
    assert list(sig.parameters)[:2] == ["path_gt", "path_generated"] and sig.parameters["save_l2"].default is False
    u8 = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(TypeError, match="quantize_image"):
        nerf.image_metrics(u8.float(), u8)
    with pytest.raises(ValueError):
        nerf.image_metrics(u8, torch.zeros(8, 9, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        nerf.image_metrics(torch.zeros(6, 8, 3, dtype=torch.uint8), torch.zeros(6, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        nerf.image_metrics(torch.zeros(8, 6, 3, dtype=torch.uint8), torch.zeros(8, 6, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        nerf.image_metrics(u8, u8)


def test_metrics_file_layout(tmp_path):
    from nerf import metrics
    path = os.path.join(str(tmp_path), "metrics.txt")
    means = metrics.write_metrics_file(path, [("0000.png", 0.25, 10.0, 0.5), ("0001.png", 0.75, 30.0, 0.7)], "gt", "gen")
    assert means == {"frames": 2, "mean_l1": 0.5, "mean_psnr": 20.0, "mean_ssim": 0.6}
    text = open(path).read()
    lines = text.splitlines()
    assert lines[0].startswith("#") and "LPIPS" in lines[0] and "LPIPS" not in text[len(lines[0]):]
    assert lines[1:5] == ["0000.png   L1:  \t0.250000 ", "0000.png   PSNR:\t10.000000 ", "0000.png   SSIM:\t0.500000 ", ""]
    assert lines[9] == "=" * 80 and lines[10:13] == [" Summary ", " folder 1: gt ", " folder 2: gen "] and lines[13] == "-" * 80
    assert lines[14:] == [" mean L1:\t0.500000", " mean PSNR:\t20.000000", " mean SSIM:\t0.600000"]


def test_gather_rows_is_sorted_identity_at_world_size_one():
    from nerf import distributed as D
    assert D.gather_rows([(2, 0.5), (0, 0.25)]) == [(0, 0.25), (2, 0.5)]

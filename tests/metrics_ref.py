"""float64 restatement of the image metrics (L1, MSE, PSNR, SSIM of uint8 images (H, W, 3) as float images byte / 255), the
yardstick of tests/test_metrics_host.py and tests/test_gpu_image_metrics.py.

SSIM is skimage's compare_ssim(im1, im2, multichannel=True) of that generation on float input: per channel a 7 x 7 uniform window
(NP = 49), sample covariance (factor NP / (NP - 1)), C1 = (0.01 R)^2, C2 = (0.03 R)^2, S averaged over the pixels whose window lies
inside the image (3 cropped on every side), then over the channels; R = 2 is what that skimage takes for float images (dmax - dmin
of the dtype range (-1, 1)), R = 1 the textbook value.  Two forms:

* metrics_int: window sums in int64 (exact), then the formula in float64;
* ssim_uniform_filter: the way skimage computes it, scipy.ndimage.uniform_filter of the float images and of their products.
"""
import numpy as np

WIN, NP = 7, 49


def box_sums(plane: np.ndarray) -> np.ndarray:
    """(H, W, C) int64 -> (H - 6, W - 6, C): sums over every 7 x 7 window that lies inside the image (exact; rows, then columns)."""
    h, w = plane.shape[:2]
    rows = np.zeros((h, w - WIN + 1) + plane.shape[2:], dtype=np.int64)
    for dx in range(WIN):
        rows += plane[:, dx:dx + w - WIN + 1]
    acc = np.zeros((h - WIN + 1, w - WIN + 1) + plane.shape[2:], dtype=np.int64)
    for dy in range(WIN):
        acc += rows[dy:dy + h - WIN + 1]
    return acc


def window_stats(a: np.ndarray, b: np.ndarray):
    """The five exact window sums (x, y, x^2, y^2, xy) of a uint8 image pair."""
    x, y = a.astype(np.int64), b.astype(np.int64)
    return box_sums(x), box_sums(y), box_sums(x * x), box_sums(y * y), box_sums(x * y)


def ssim_map_int(a: np.ndarray, b: np.ndarray, data_range: float = 2.0, stats=None) -> np.ndarray:
    """S per valid window origin and channel, (H - 6, W - 6, 3) float64, from exact integer window statistics."""
    sx, sy, sxx, syy, sxy = window_stats(a, b) if stats is None else stats
    ux, uy = sx / (NP * 255.0), sy / (NP * 255.0)
    m = (NP - 1) * NP * 255.0 * 255.0                       # vx = (NP / (NP - 1)) (sum x^2 / NP - ux^2), over a common denominator
    vx, vy, vxy = (NP * sxx - sx * sx) / m, (NP * syy - sy * sy) / m, (NP * sxy - sx * sy) / m
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def metrics_int(a: np.ndarray, b: np.ndarray, data_range: float = 2.0, stats=None) -> dict:
    """One image pair (H, W, 3) uint8 -> {"abs_sum", "sq_sum"} (python ints) and {"l1", "mse", "psnr", "ssim"} (float64)."""
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 3 and a.shape[2] == 3
    d = a.astype(np.int64) - b.astype(np.int64)
    abs_sum, sq_sum = int(np.abs(d).sum()), int((d * d).sum())
    count = float(d.size)
    mse = np.float64(sq_sum) / (65025.0 * count)
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(np.float64(1.0) / mse)
    s = ssim_map_int(a, b, data_range, stats)
    ssim = np.mean([s[..., c].mean() for c in range(3)])
    return {"abs_sum": abs_sum, "sq_sum": sq_sum, "l1": np.float64(abs_sum) / (255.0 * count), "mse": mse, "psnr": psnr, "ssim": np.float64(ssim)}


def ssim_uniform_filter(a: np.ndarray, b: np.ndarray, data_range: float = 2.0) -> float:
    """The same SSIM the way skimage forms it: uniform_filter of the float64 images and their products, cropped by 3."""
    from scipy.ndimage import uniform_filter
    cov_norm = NP / (NP - 1.0)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    per_channel = []
    for c in range(3):
        x, y = a[..., c].astype(np.float64) / 255, b[..., c].astype(np.float64) / 255
        ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
        uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        per_channel.append(s[3:-3, 3:-3].mean())
    return float(np.mean(per_channel))


def ssim_skimage(a: np.ndarray, b: np.ndarray, data_range: float = 2.0):
    """skimage's own figure where the package is installed (either generation of its interface), else None."""
    try:
        import skimage  # noqa: F401
    except ImportError:
        return None
    x, y = a.astype(np.float64) / 255, b.astype(np.float64) / 255
    try:
        from skimage.metrics import structural_similarity
        try:
            return float(structural_similarity(x, y, channel_axis=2, data_range=data_range))
        except TypeError:
            return float(structural_similarity(x, y, multichannel=True, data_range=data_range))
    except ImportError:
        from skimage.measure import compare_ssim
        return float(compare_ssim(x, y, multichannel=True, data_range=data_range))


# ---- image contents shared by the host and the GPU tests (seeded; (H, W, 3) uint8 pairs)
def random_pair(h, w, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8), rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


def gradient_pair(h, w, seed, noise=12.0):
    """A smooth colour gradient and the same gradient with noise: SSIM in mid-range."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([255 * xx / max(w - 1, 1), 255 * yy / max(h - 1, 1), 127.5 + 127.5 * np.sin(0.2 * xx + 0.13 * yy)], axis=-1)
    a = np.clip(np.round(base), 0, 255).astype(np.uint8)
    b = np.clip(np.round(base + noise * rng.randn(h, w, 3)), 0, 255).astype(np.uint8)
    return b, a


def identical_pair(h, w, seed):
    a, _ = random_pair(h, w, seed)
    return a, a.copy()


def black_white_pair(h, w, seed=0):
    return np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)


def one_pixel_pair(h, w, seed, y, x, channel=1, delta=37):
    """A gradient image and a copy with one byte changed by `delta` at (y, x, channel)."""
    _, a = gradient_pair(h, w, seed)
    b = a.copy()
    b[y, x, channel] = (int(a[y, x, channel]) + delta) % 256
    return b, a

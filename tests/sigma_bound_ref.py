"""Host restatement of the sigma gate (csrc/nf_mlp_gated.hip, DESIGN.md "Sigma gate"): the folded fc_alpha . fc_feat row and its
absolute-value twin, and the test that proves a sample dead from h = relu(layers_xyz.5) alone.  NumPy / torch on the CPU; the
kernel's MFMA sums the same 257 terms in another order, which the bound's slack covers, so the restatement and the kernel
agree on every row that is not within that slack of the threshold -- the GPU tests compare them with the coefficient doubled."""
import numpy as np
import torch

from oracle import nerface_oracle as O

COEF = 2.0 ** -13          # the kernel's: 2048 u, u = 2^-24
ABS = 2.0 ** -100


def _round_up(x64):
    """float64 -> the next float32 at or above (NaN stays NaN, +inf stays +inf)."""
    f = x64.astype(np.float32)
    with np.errstate(invalid="ignore"):
        low = f.astype(np.float64) < x64
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def bound_vectors(p):
    """(w, c, v, d) of one weight set (a dict of float32 tensors by state_dict name): w = a^T F, c = a . f + b to nearest; v = |a|^T |F|,
    d = |a| . |f| + |b| rounded up; all four computed in float64."""
    a = p["fc_alpha.weight"].detach().cpu().numpy().astype(np.float64).reshape(-1)
    b = float(p["fc_alpha.bias"].detach().cpu().numpy().astype(np.float64).reshape(-1)[0])
    F = p["fc_feat.weight"].detach().cpu().numpy().astype(np.float64)
    f = p["fc_feat.bias"].detach().cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        w = (a[:, None] * F).sum(0).astype(np.float32)
        c = np.float32((a * f).sum() + b)
        v = _round_up((np.abs(a)[:, None] * np.abs(F)).sum(0))
        d = _round_up(np.asarray((np.abs(a) * np.abs(f)).sum() + abs(b)))
    return w, c, v, np.float32(d)


def gate(h, w, c, v, d, coef=COEF):
    """h: (P, 256) float32, relu(layers_xyz.5) -> (s, u, bound, proven): s = w . h + c and u = v . h + d accumulated in float32, bound =
    s + coef u, proven = bound < -2^-100 with finite operands.  (A ray's last sample is the caller's business.)"""
    h = np.asarray(h, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (h @ w.astype(np.float32) + np.float32(c)).astype(np.float32)
        u = (h @ v.astype(np.float32) + np.float32(d)).astype(np.float32)
        bound = (s + np.float32(coef) * u).astype(np.float32)
        proven = (bound < np.float32(-ABS)) & np.isfinite(s) & np.isfinite(u)
    return s, u, bound, proven


def trunk(p, x87, expr, latent, dtype=torch.float32):
    """(h, sigma): relu(layers_xyz.5) and sigma_raw of the oracle's paper MLP on pre-encoded points, in `dtype`."""
    q = {k: t.detach().cpu().to(dtype) for k, t in p.items()}
    acts = []
    with torch.no_grad():
        raw = O.paper_mlp(q, x87.to(dtype), expr.cpu().to(dtype), latent.cpu().to(dtype), acts=acts)
    return acts[5], raw[:, 3]


def cancelling(p, x87, expr, latent):
    """The cancelling net of `p`: fc_alpha.weight x 1e-3 and fc_alpha.bias set so that the median sigma_raw of the given points is
    about 0: the densities crowd around zero, half on either side, where a wrong sign would show.  (The scale leaves s / u as it
    was, so the gate still proves most dead rows; it must prove none wrongly.)"""
    q = {k: t.clone() for k, t in p.items()}
    q["fc_alpha.weight"] = q["fc_alpha.weight"] * 1.0e-3
    q["fc_alpha.bias"] = torch.zeros_like(q["fc_alpha.bias"])
    _, sigma = trunk(q, x87, expr, latent, torch.float64)
    q["fc_alpha.bias"] = torch.full_like(q["fc_alpha.bias"], -float(sigma.median()))
    return q


def benchmark_shares(frames, rays):
    """For tools/sigma_bound_check.py: with the benchmark's weights, poses, conditioning and validation settings (bench_common) and
    `rays` random rays of each frame, yields (frame, (live share, not-proven share) of the coarse pass, the same of the fine pass,
    proven points with positive float64 density)."""
    import bench_common as BC
    cpu = torch.device("cpu")
    nets = [{k: v.detach().clone() for k, v in BC.synth_params(s, cpu).state_dict().items()} for s in (0, 1)]
    vecs = [bound_vectors(p) for p in nets]

    def shares(p, vec, ro, rd, z, expr, latent):
        x87 = O.encode_points(ro, rd, z, BC.NEAR, BC.FAR)
        h, sigma = trunk(p, x87, expr, latent)
        proven = gate(h.numpy(), *vec)[3]
        s = z.shape[1]
        proven[s - 1::s] = False
        q = {k: p[k].double() for k in ("fc_feat.weight", "fc_feat.bias", "fc_alpha.weight", "fc_alpha.bias")}
        sigma64 = ((h.double() @ q["fc_feat.weight"].t() + q["fc_feat.bias"]) @ q["fc_alpha.weight"].t() + q["fc_alpha.bias"]).reshape(-1).numpy()
        wrong = int((proven & (sigma64 > 0)).sum())
        live = ~(sigma.numpy() <= 0)
        live[s - 1::s] = True
        return float(live.mean()), float(1.0 - proven.mean()), wrong, sigma.reshape(z.shape)

    for f in frames:
        g = torch.Generator().manual_seed(1000 + f)
        expr, latent = 0.5 * torch.randn(76, generator=g), 0.1 * torch.randn(32, generator=g)
        ro, rd = O.ray_bundle(BC.H, BC.W, BC.INTRINSICS, BC.frame_pose(f))
        pick = torch.randperm(BC.H * BC.W, generator=g)[:rays]
        ro, rd = ro.reshape(-1, 3)[pick], rd.reshape(-1, 3)[pick]
        z_c = O.coarse_z(rays, BC.NEAR, BC.FAR, BC.N_COARSE, torch.rand((rays, BC.N_COARSE), generator=g))
        live_c, kept_c, wrong_c, sigma_c = shares(nets[0], vecs[0], ro, rd, z_c, expr, latent)
        raw = torch.cat((torch.zeros(rays, BC.N_COARSE, 3), sigma_c[..., None]), dim=-1)
        w_c = O.volume_render(raw, z_c, rd, None, has_background=False)[3]
        z_s = O.sample_pdf(0.5 * (z_c[:, 1:] + z_c[:, :-1]), w_c[:, 1:-1], BC.N_FINE, torch.rand((rays, BC.N_FINE), generator=g))
        z_f = torch.sort(torch.cat((z_c, z_s), dim=-1), dim=-1)[0]
        live_f, kept_f, wrong_f, _ = shares(nets[1], vecs[1], ro, rd, z_f, expr, latent)
        yield f, (live_c, kept_c), (live_f, kept_f), wrong_c + wrong_f

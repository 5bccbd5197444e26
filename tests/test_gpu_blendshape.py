"""The two blendshape classes without a learnable code (ConditionalBlendshapeNeRFModel = "bshape", ConditionalCompressedBlendshapeNeRFModel
= "cbshape") on the second family's kernels: parity against the reference's golden outputs / gradients (tests/golden/bshape_*.npz,
cbshape_*.npz), the float64 restatement (tests/blendshape_ref.py) and -- bit for bit -- the second family itself.  GPU only.
Every tolerance is the one the project already holds the second family to for the same quantity (tests/test_gpu_lcode.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import blendshape_ref as B
from tests import util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
PRECISIONS = ["f32", "f16x3", "bf16x3", "f16x2"]


@pytest.fixture(autouse=True)
def _f32_afterwards():
    import nerf
    yield
    nerf.set_mlp_precision("f32")


def maker(kind):
    def make(nerf, params, device):
        m = getattr(nerf.models, B.CLASS[kind])(**B.MODEL_KW)
        assert list(m.state_dict().keys()) == B.KEYS[kind]
        m.load_state_dict(params)
        return m.to(device)
    return make


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _points(n_rays, s, seed, frame=3):
    g = torch.Generator().manual_seed(seed)
    ro, rd, _, _, _ = C.ray_subset(512, 512, frame, n_rays, seed + 7)
    z = torch.sort(torch.rand((n_rays, s), generator=g) * 0.6 + 0.2, dim=-1)[0]
    return ro, rd, z


# ---------------------------------------------------------------------------------------------------------------- 1. end to end
E2E = [(f"{kind}_{base}", "f32") for kind in B.KINDS for base in B.BASES] + [(f"{kind}_soft_eval_det_64_128", "f16x3") for kind in B.KINDS]


@pytest.mark.parametrize("name,precision", E2E)
def test_blendshape_against_golden_reference(hip_lib, gpu, name, precision):
    """run_one_iter_of_nerf against the unmodified reference's outputs, every element within the copied tolerance; the eval case
    also in "f16x3" at the same f32 tolerances."""
    import nerf
    c = B.build_case(name)
    gold = np.load(os.path.join(GOLD, f"{name}.npz"))
    assert abs(float(gold["params_checksum"]) - B.checksum(c)) < 1e-6
    nerf.set_mlp_precision(precision)
    out, _, _, _ = U.run_product(nerf, c, gpu, make=maker(c["kind"]))
    tol = B.case_tol(name)
    worst = {}
    for n, t in zip(B.NAMES7, out):
        if t is None:
            assert n not in gold.files
            continue
        worst[n] = float(np.abs(t.cpu().numpy() - gold[n]).max())
        print(f"[{name} {precision}] {n}: max|d|={worst[n]:.3e} (gate {tol[n]:.0e})")
    for n, d in worst.items():
        assert d <= tol[n], (name, precision, n, d)


# ---------------------------------------------------------------------------------------------------------------- 2. MLP alone
# per output column, against the float64 restatement: the bounds of test_lcode_mlp_vs_fp64_oracle ("f32"),
# test_lcode_f16x3_mlp_meets_the_f32_gate, test_lcode_bf16x3_mlp_vs_oracle and tests/test_gpu_f16x2.py (rgb 1e-3, sigma 2e-3 T with
# T = max over points of sqrt(sum_k (x_k fc_alpha.weight_k)^2), x = fc_alpha's input)
def mlp_bound(precision, scale, t_sigma):
    if precision in ("f32", "f16x3"):
        return 2e-5 * scale + 2e-5
    if precision == "bf16x3":
        return 3e-4 * scale + 1e-5
    return torch.tensor([1e-3, 1e-3, 1e-3, 2e-3 * t_sigma], dtype=torch.float64)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n_rays,s", [(5, 7), (7, 37)])            # 35 points; 259 = 4 x 64 + 3 points
@pytest.mark.parametrize("kind", B.KINDS)
def test_blendshape_mlp_vs_fp64_restatement(hip_lib, gpu, kind, n_rays, s, precision):
    import nerf
    c = B.build_case(f"{kind}_soft_eval_det_64_128")
    ro, rd, z = _points(n_rays, s, 2)
    p = B.init_params(kind, 14, boost="survey")
    m = maker(kind)(nerf, p, gpu)
    assert m.fused_supported()
    nerf.set_mlp_precision(precision)
    raw, state = m.hip_forward(ro.to(gpu), rd.to(gpu), z.to(gpu), None, c["expr"].to(gpu), c["latent"].to(gpu), O.NEAR, O.FAR, False)
    assert state is None and raw.shape == (n_rays, s, 4)
    p64 = {k: v.double() for k, v in p.items()}
    acts = []
    ref = B.MLP[kind](p64, O.encode_points(ro, rd, z, O.NEAR, O.FAR).double(), c["expr"].double(), acts=acts)
    t_sigma = float(((acts[3] ** 2) @ (p64["fc_alpha.weight"] ** 2).t()).sqrt().max())          # acts[3]: layers_xyz.2's output
    scale = ref.abs().amax(dim=0)
    err = (raw.cpu().reshape(-1, 4).double() - ref).abs().amax(dim=0)
    print(f"{kind} {precision} hip_forward ({n_rays}x{s}) err", err.tolist(), "scale", scale.tolist(), "T", t_sigma)
    assert torch.all(err <= mlp_bound(precision, scale, t_sigma))
    other = m.hip_forward(ro.to(gpu), rd.to(gpu), z.to(gpu), None, c["expr"].to(gpu), torch.ones(32, device=gpu), O.NEAR, O.FAR, False)[0]
    assert torch.equal(other, raw)                                   # the latent code has no effect on the output


# ---------------------------------------------------------------------------------------------------------------- 3. bit identity
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bshape_equals_second_family_with_zero_latent_columns_bitwise(hip_lib, gpu, precision):
    """A second-family model with layer1.weight = [W[:, :139] | 0 (32)] and every other tensor shared, under a non-zero latent code:
    raw and -- after a backward with the same d_raw -- every shared gradient and layer1.weight.grad[:, :139] equal the bshape
    model's bit for bit.  Pins the pack tables, the bias table and the gradient scatter of nf_bshape_* in one stroke."""
    import nerf
    c = B.build_case("bshape_soft_train_rand_64_64")
    p = B.init_params("bshape", 14, boost="survey")
    pl = dict(p)
    pl["layer1.weight"] = torch.cat((p["layer1.weight"], torch.zeros(256, 32)), dim=1)
    mb, ml = maker("bshape")(nerf, p, gpu), U.make_lcode_model(nerf, pl, gpu)
    n_rays, s = 7, 37
    ro, rd, z = _points(n_rays, s, 5)
    g = torch.Generator().manual_seed(3)
    d_raw = torch.randn((n_rays, s, 4), generator=g).to(gpu)
    latent = c["latent"].to(gpu)
    assert float(latent.abs().min()) > 0
    args = (ro.to(gpu), rd.to(gpu), z.to(gpu), None, c["expr"].to(gpu), latent, O.NEAR, O.FAR)
    nerf.set_mlp_precision(precision)
    assert torch.equal(mb.hip_forward(*args, False)[0], ml.hip_forward(*args, False)[0])
    if precision == "f16x2":                                        # inference arithmetic
        return
    (raw_b, st_b), (raw_l, st_l) = mb.hip_forward(*args, True), ml.hip_forward(*args, True)
    assert torch.equal(raw_b, raw_l)
    (gb, lat_b), (gl, _) = mb.hip_backward(st_b, z.to(gpu), d_raw), ml.hip_backward(st_l, z.to(gpu), d_raw)
    assert torch.equal(lat_b, torch.zeros(32, device=gpu))
    for k, a, b in zip(B.KEYS["bshape"], gb, gl):
        assert torch.equal(a, b[:, :139] if k == "layer1.weight" else b), k
        assert float(a.abs().max()) > 0, k


# ---------------------------------------------------------------------------------------------------------------- 4. gradients
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("kind", B.KINDS)
def test_blendshape_train_step_vs_reference_gradients(hip_lib, gpu, kind, precision):
    """The end-to-end training step through run_one_iter_of_nerf + nerf.training_loss against the unmodified reference's fp32 autograd
    (a frame without a ReLU decision within fp32 rounding, the encoder included): rel-L2 1e-4 per tensor, the project's gate for "f32"
    and "f16x3".  The fixture stores the tensors of up to 4096 elements whole (all six layers_expr tensors of both models among
    them) and norm + 257-element head of the larger ones (size limit of a committed file); the latent code's gradient equals the
    regulariser's alone."""
    import nerf
    name = B.GRAD_CASES[kind]
    c = B.build_case(name)
    gold = np.load(os.path.join(GOLD, f"{name}_grads.npz"))
    assert abs(float(gold["params_checksum"]) - B.checksum(c)) < 1e-6
    nerf.set_mlp_precision(precision)
    out, mc, mf, latent = U.run_product(nerf, c, gpu, grad=True, make=maker(kind))
    with torch.enable_grad():
        loss, _ = nerf.training_loss(out[0], out[3], c["tgt"].to(gpu), latent)
        loss.backward()
    d_loss = abs(float(loss.detach()) - float(gold["loss"]))
    lat = c["latent"].double()
    e_reg = rel_l2(latent.grad.cpu(), 10 * 0.0005 * lat / lat.norm())
    e_lat = rel_l2(latent.grad.cpu(), torch.from_numpy(gold["latent"]))
    print(f"{kind} {precision} train step: |d loss| {d_loss:.2e}, latent vs regulariser {e_reg:.2e}, vs reference {e_lat:.2e}")
    assert d_loss <= 1e-4 * abs(float(gold["loss"])) and e_reg < 1e-6 and e_lat < 1e-4
    worst, n_full = {}, 0
    for tag, m in (("coarse", mc), ("fine", mf)):
        for k, v in m.named_parameters():
            assert v.grad is not None and bool(torch.isfinite(v.grad).all()), (tag, k)
            want = float(gold[f"norm:{tag}.{k}"])
            e = abs(float(v.grad.double().norm()) - want) / want
            if f"full:{tag}.{k}" in gold.files:
                e = max(e, rel_l2(v.grad.cpu(), torch.from_numpy(gold[f"full:{tag}.{k}"])))
                n_full += 1
            else:
                e = max(e, rel_l2(v.grad.reshape(-1)[:257].cpu(), torch.from_numpy(gold[f"head:{tag}.{k}"])))
            worst[f"{tag}.{k}"] = e
    print(f"{kind} {precision} train step: worst gradient rel error", max(worst.values()), max(worst, key=worst.get))
    assert n_full >= (2 * 14 if kind == "cbshape" else 2 * 8)
    for k, e in worst.items():
        assert e < 1e-4, (k, e)


@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16x3"])
def test_cbshape_mlp_bwd_vs_fp64_restatement(hip_lib, gpu, precision):
    """MLP-level gradients of all 22 tensors on 35 points against float64 autograd of the restatement evaluated at the trunk ReLU masks
    the HIP forward saw (the encoder runs free: its units are checked to be away from zero), the encoder tensors reported separately.
    rel-L2 1e-4 per tensor; bf16x3: the 3e-4 of test_lcode_mlp_bwd_vs_fp64_oracle."""
    import nerf
    from nerf import ops
    tol = 3e-4 if precision == "bf16x3" else 1e-4
    c = B.build_case("cbshape_soft_train_rand_64_64")
    n_rays, s = 5, 7
    g = torch.Generator().manual_seed(23)
    ro, rd, _, _, _ = C.ray_subset(512, 512, 9, n_rays, 23)
    z = torch.sort(torch.rand((n_rays, s), generator=g) * 0.6 + 0.2, dim=-1)[0]
    d_raw = torch.randn((n_rays, s, 4), generator=g)
    p = B.init_params("cbshape", 14, boost="survey")
    m = maker("cbshape")(nerf, p, gpu)
    args = (ro.to(gpu), rd.to(gpu), z.to(gpu), rd.to(gpu), c["expr"].to(gpu), c["latent"].to(gpu), O.NEAR, O.FAR)
    nerf.set_mlp_precision(precision)
    raw_e, _ = m.hip_forward(*args, False)
    raw_t, state = m.hip_forward(*args, True)
    assert torch.equal(raw_t, raw_e)                       # training forward == eval forward, bit for bit
    grads, g_lat = m.hip_backward(state, z.to(gpu), d_raw.to(gpu))
    assert len(grads) == 22 and all(gh is not None for gh in grads) and torch.equal(g_lat, torch.zeros(32, device=gpu))
    n_pts = n_rays * s
    sv = state[2]
    if precision != "f32":
        sv = ops.split_saved_to_f32(sv, n_pts, f16=precision == "f16x3", family="lcode")     # the second family's layout
    sv = sv.cpu()
    secs = dict(x0=(320, 256), x1=(576, 256), x2=(832, 256), feat=(1088, 256), dir=(1344, 128))     # csrc/nf_mlp_lcode_layout.h: S_*
    masks = [sv[o * n_pts:(o + w) * n_pts].view(n_pts, w) > 0 for o, w in secs.values()]
    pp = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
    enc_acts = []
    out = B.cbshape_mlp(pp, O.encode_points(ro.double(), rd.double(), z.double(), O.NEAR, O.FAR), c["expr"].double(), masks=masks,
                        enc_acts=enc_acts)
    out.backward(d_raw.reshape(-1, 4).double())
    for e in enc_acts:                                     # active and inactive units in every encoder layer, none at a rounding's distance
        on = e.detach() > 0
        assert bool(on.any()) and not bool(on.all()) and float(e.detach()[on].min()) > 1e-5
    # the bias table's corner holds the encoder's activations (csrc/nf_mlp_bshape.h: ncb::C_E1 ..)
    cond = state[1].cpu()
    for off, e in zip((1564 + 76, 1564 + 76 + 38, 1564 + 76 + 38 + 20), enc_acts):
        assert (cond[off:off + e.numel()].double() - e.detach().reshape(-1)).abs().max() < 1e-5
    worst = {"encoder": 0.0, "trunk": 0.0}
    for k, gh in zip(B.KEYS["cbshape"], grads):
        e = rel_l2(gh.cpu(), pp[k].grad)
        part = "encoder" if k.startswith("layers_expr") else "trunk"
        worst[part] = max(worst[part], e)
        assert e < tol, (k, e)
    print(f"cbshape {precision} mlp bwd ({n_rays}x{s}): worst rel L2", worst)


# ---------------------------------------------------------------------------------------------------------------- 5. forward(x87)
@pytest.mark.parametrize("kind", B.KINDS)
def test_blendshape_forward_and_run_network(hip_lib, gpu, kind):
    """model.forward(x87, expr) -- with and without a latent code -- and nerf.run_network against the float64 restatement (the gates of
    test_lcode_model_forward_and_run_network_on_encoded_inputs); autograd through forward is refused; a 75-element expression raises
    ValueError before any launch."""
    import nerf
    c = B.build_case(f"{kind}_soft_eval_det_64_128")
    n_rays, s = 6, 37
    ro, rd, z = _points(n_rays, s, 2)
    p = B.init_params(kind, 14, boost="survey")
    m = maker(kind)(nerf, p, gpu)
    expr, lat = c["expr"].to(gpu), c["latent"].to(gpu)
    x87 = O.encode_points(ro, rd, z, O.NEAR, O.FAR)
    ref = B.MLP[kind]({k: v.double() for k, v in p.items()}, x87.double(), c["expr"].double())
    scale = ref.abs().amax(dim=0)
    with torch.no_grad():
        out = m(x87.to(gpu), expr)
        assert torch.equal(out, m(x87.to(gpu), expr, lat)) and torch.equal(out, m(x87.to(gpu), expr, latent_code=lat))
        assert m(x87[:0].to(gpu), expr).shape == (0, 4)
    err = (out.cpu().double() - ref).abs().amax(dim=0)
    print(f"{kind} forward(x87) err", err.tolist(), "scale", scale.tolist())
    assert out.shape == (n_rays * s, 4) and torch.all(err <= 2e-5 * scale + 2e-5)
    ex, ed = U.encoders(nerf)
    pts = (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).to(gpu)
    ray_batch = torch.cat((ro, rd, torch.full((n_rays, 1), O.NEAR), torch.full((n_rays, 1), O.FAR)), dim=-1).to(gpu)
    with torch.no_grad():
        for latent in (lat, None):
            rf = nerf.run_network(m, pts, ray_batch, 100, ex, ed, expr, latent).cpu()
            assert rf.shape == (n_rays, s, 4)
            assert torch.all((rf.reshape(-1, 4).double() - ref).abs().amax(dim=0) <= 3e-5 * scale + 3e-5)
    with pytest.raises(NotImplementedError, match="no autograd"):
        m(x87.to(gpu), expr)
    hw = maker(kind)(nerf, p, gpu)
    with pytest.raises(ValueError), torch.no_grad():
        hw(x87.to(gpu), expr[:75])
    with pytest.raises(ValueError):
        hw.hip_forward(ro.to(gpu), rd.to(gpu), z.to(gpu), None, expr[:75], lat, O.NEAR, O.FAR, False)
    assert hw.__dict__.get("_hip_weights") is None or hw.hip_weights()._cache == {}          # refused before anything was packed


# ---------------------------------------------------------------------------------------------------------------- 6. launchers
def test_launchers_compressed_blendshape_model(hip_lib, gpu, tmp_path):
    """launch.train_sharded for three iterations, then launch.eval_sharded in "f32" and "f16x3", with
    `type: ConditionalCompressedBlendshapeNeRFModel` in the config (as the six `*_compressed` configs have): all 22 tensors of both
    models move, the loss is finite, the renders are not constant."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))
    import make_synthetic_dataset as MS
    from launch import eval_sharded, train_sharded
    from PIL import Image
    base = str(tmp_path)
    MS.write(os.path.join(base, "data"))
    cfg_path = os.path.join(base, "config.yml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(MS.config(os.path.join(base, "data"), os.path.join(base, "logs"), train_iters=3,
                                 model_type="ConditionalCompressedBlendshapeNeRFModel"), f)
    logdir = train_sharded.main(["--config", cfg_path])
    ck0 = torch.load(os.path.join(logdir, "checkpoint00000.ckpt"), map_location="cpu")
    ck_path = os.path.join(logdir, "checkpoint00002.ckpt")
    ck = torch.load(ck_path, map_location="cpu")
    keys = B.KEYS["cbshape"]
    for sd in ("model_coarse_state_dict", "model_fine_state_dict"):
        assert list(ck[sd].keys()) == keys
        still = [k for k in keys if torch.equal(ck[sd][k], ck0[sd][k])]
        assert not still, (sd, still)                                 # every tensor of the class receives gradients
    assert np.isfinite(float(ck["loss"]))
    for precision in ("f32", "f16x3"):
        out = os.path.join(base, "render_" + precision)
        assert eval_sharded.main(["--config", cfg_path, "--checkpoint", ck_path, "--savedir", out, "--precision", precision]) == [0, 1, 2]
        a = np.asarray(Image.open(os.path.join(out, "0001.png")))
        assert a.shape == (32, 32, 3) and a.std() > 0

"""Third model family (ConditionalBlendshapePaperSmallerNeRFModel, reference nerf/models.py:266-338): its restatement, its seeded
cases, and the generator of tests/golden/smaller_*.npz.  TEST INFRASTRUCTURE ONLY.

Regenerate the fixtures where the unmodified reference can be imported (oracle/ref_import.py):   python -m tests.smaller_ref
The fixtures hold reference OUTPUTS (arrays only); inputs and weights are regenerated from seeds, a weight checksum detects drift.
`python -m tests.smaller_ref search` prints how the seeds and frames below were chosen.
"""
from __future__ import annotations

import math
import os
import sys
from typing import Dict, Optional, Sequence

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import cases as C                      # noqa: E402
from oracle import nerface_oracle as O             # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAMES7 = ["rgb_c", "disp_c", "acc_c", "rgb_f", "disp_f", "acc_f", "w_last"]

SMALLER_SHAPES = {
    "layers_xyz.0.weight": (256, 171), "layers_xyz.1.weight": (256, 256), "layers_xyz.2.weight": (256, 256),
    "layers_xyz.3.weight": (256, 427), "layers_xyz.4.weight": (256, 256),
    "fc_feat.weight": (256, 256), "fc_alpha.weight": (1, 256),
    "layers_dir.0.weight": (128, 356), "layers_dir.1.weight": (128, 128), "layers_dir.2.weight": (128, 128),
    "fc_rgb.weight": (3, 128),
}
SMALLER_KEYS = [k.replace("weight", p) for k in SMALLER_SHAPES for p in ("weight", "bias")]          # state_dict order
SMALLER_NUMEL = sum(s[0] * s[1] + s[0] for s in SMALLER_SHAPES.values())                                # 496,132
SMALLER_KW = dict(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=False, use_viewdirs=True,
                  num_layers=4, hidden_size=256, include_expression=True)                               # as the two configs construct it


def init_smaller_params(seed: int, dtype=torch.float32, boost=True) -> Dict[str, torch.Tensor]:
    """Seeded like O.init_lcode_params: nn.Linear-style uniform init from an own generator; boost="survey": SURVEY 8(d)'s density head
    (fc_alpha.weight x40, bias 0.5), boost=True: the hard head (x300, bias 5); fc_rgb.weight x10 in both."""
    g = torch.Generator().manual_seed(seed)
    out: Dict[str, torch.Tensor] = {}
    for k, shp in SMALLER_SHAPES.items():
        bound = 1.0 / math.sqrt(shp[1])
        out[k] = ((torch.rand(shp, generator=g, dtype=torch.float64) * 2 - 1) * bound).to(dtype)
        out[k.replace("weight", "bias")] = ((torch.rand(shp[0], generator=g, dtype=torch.float64) * 2 - 1) * bound).to(dtype)
    if boost == "survey":
        out["fc_alpha.weight"] = out["fc_alpha.weight"] * 40.0
        out["fc_alpha.bias"] = torch.full_like(out["fc_alpha.bias"], 0.5)
        out["fc_rgb.weight"] = out["fc_rgb.weight"] * 10.0
    elif boost:
        out["fc_alpha.weight"] = out["fc_alpha.weight"] * 300.0
        out["fc_alpha.bias"] = torch.full_like(out["fc_alpha.bias"], 5.0)
        out["fc_rgb.weight"] = out["fc_rgb.weight"] * 10.0
    return out


def smaller_mlp(p: Dict[str, torch.Tensor], x87: torch.Tensor, expr: torch.Tensor, latent: torch.Tensor,
                masks: Optional[Sequence[torch.Tensor]] = None, acts: Optional[list] = None) -> torch.Tensor:
    """ConditionalBlendshapePaperSmallerNeRFModel.forward (M:313-338): (P, 87) -> (P, 4) = [rgb_raw, sigma_raw].

    x0 = [pe_xyz(63) | expr*1/3 (76) | latent (32)]; 3x(Linear+ReLU); skip-concat [x0 | h] at layer 3; 1x(Linear+ReLU);
    feat = fc_feat(h) (no activation); sigma = fc_alpha(feat); [feat | pe_dir(24) | expr*1/3 (76)] -> layers_dir.0..2 (+ReLU);
    rgb = fc_rgb.  Test hooks as O.paper_mlp: `masks` (8 boolean tensors: layers_xyz.0..4, layers_dir.0..2) replaces each ReLU by a
    multiplication with the given mask; `acts` (a list) collects the 5 + 3 post-ReLU activations, with feat after the first five."""
    n = x87.shape[0]
    xyz, dirs = x87[:, :63], x87[:, 63:]
    e = (expr * 1 / 3).reshape(1, -1).repeat(n, 1)              # true division, M:318
    l = latent.reshape(1, -1).repeat(n, 1)
    x0 = torch.cat((xyz, e, l), dim=1)
    k = [0]

    def act(v):
        out = torch.relu(v) if masks is None else v * masks[k[0]].to(v.dtype)
        k[0] += 1
        if acts is not None:
            acts.append(out)
        return out

    h = x0
    for i in range(5):
        h = act(O._lin(torch.cat((x0, h), dim=-1) if i == 3 else h, p, f"layers_xyz.{i}"))
    feat = O._lin(h, p, "fc_feat")
    if acts is not None:
        acts.append(feat)
    sigma = O._lin(feat, p, "fc_alpha")
    h = act(O._lin(torch.cat((feat, dirs, e), dim=-1), p, "layers_dir.0"))
    h = act(O._lin(h, p, "layers_dir.1"))
    h = act(O._lin(h, p, "layers_dir.2"))
    rgb = O._lin(h, p, "fc_rgb")
    return torch.cat((rgb, sigma), dim=-1)


# ---- gates: the tables tests/test_gpu_e2e.py holds the paper family to, per density head (copied, not imported: a GPU test module) ----
TOL = dict(rgb_c=3e-6, rgb_f=3e-4, acc_c=1e-5, acc_f=1e-5, w_last=5e-4, disp_c=1e-5, disp_f=5e-5)          # hard head
TOL_SOFT = dict(rgb_c=3e-6, rgb_f=2e-5, acc_c=1e-5, acc_f=1e-5, w_last=1e-5, disp_c=2e-5, disp_f=2e-5)     # survey head

# name: ray / sample geometry as oracle/cases.py's case `base`, on `frame`, with weights init_smaller_params(seeds[0 | 1], boost).
# Seeds and frames: the first of the scanned candidates (`search`) on which the reference's own fp32 result lies within a third of
# every output's gate of the float64 restatement -- so that a product within fp32 rounding of the exact result passes the gate.
SMALLER_CASES = {
    "smaller_soft_eval_det_64_128": dict(base="soft_eval_det_64_128", frame=3, seeds=(13, 14), boost="survey"),
    "smaller_soft_train_rand_64_64": dict(base="soft_train_rand_64_64", frame=17, seeds=(11, 12), boost="survey"),
    "smaller_ragged_5_7": dict(base="ragged_5_7", frame=5, seeds=(13, 14), boost=True),
    "smaller_coarse_only": dict(base="coarse_only", frame=8, seeds=(11, 12), boost=True),
}
# the end-to-end GRADIENT case: few rays, soft head, a frame without a ReLU decision within fp32 rounding (`search`, as
# oracle/make_golden.py search_soft_grads, over frames 0..299: frame 193 has the third-largest smallest |ReLU input|, 4.6e-7 in
# float64, and the reference's fp32 autograd equals the float64 autograd to 5.6e-6 in every tensor)
GRAD_CASE = "smaller_soft_train_noflip_64_64"
SMALLER_CASES[GRAD_CASE] = dict(base="soft_train_noflip_64_64", frame=193, seeds=(13, 14), boost="survey")


def case_tol(name):
    return TOL_SOFT if SMALLER_CASES[name]["boost"] == "survey" else TOL


def build_case(name, dtype=torch.float32, **override):
    """oracle/cases.py build_case for this family: the geometry of SMALLER_CASES[name]["base"] on this case's frame and weights."""
    spec = dict(SMALLER_CASES[name], **override)
    c = dict(C.CASES[spec["base"]], frame=spec["frame"])
    c.pop("boost", None)
    ro, rd, bg, tgt, idx = C.ray_subset(512, 512, c["frame"], c["n_rays"], seed=31 + c["frame"], dtype=dtype)
    expr, latent = O.frame_conditioning(c["frame"], dtype)
    c.update(ro=ro, rd=rd, bg=bg, tgt=tgt, idx=idx, expr=expr, latent=latent)
    if c["stochastic"]:
        t_rand, noise_c, u, noise_f = C.randoms(c["n_rays"], c["n_coarse"], max(c["n_fine"], 1), dtype=dtype)
        c.update(t_rand=t_rand, u=u if c["n_fine"] > 0 else None,
                 noise_c=noise_c * c["noise_std"] if c["noise_std"] > 0 else None,
                 noise_f=noise_f * c["noise_std"] if c["noise_std"] > 0 else None, noise_c_unit=noise_c, noise_f_unit=noise_f)
    else:
        c.update(t_rand=None, u=None, noise_c=None, noise_f=None)
    c["p_coarse"] = init_smaller_params(spec["seeds"][0], dtype, boost=spec["boost"])
    c["p_fine"] = init_smaller_params(spec["seeds"][1], dtype, boost=spec["boost"])
    return c


def run_restatement(c, dtype=None, params=None, latent=None):
    """O.render_rays with this family's MLP on case `c` (dtype: evaluate everything in that type)."""
    f = (lambda t: t) if dtype is None else (lambda t: None if t is None else t.to(dtype))
    pc, pf = params if params is not None else ({k: f(v) for k, v in c["p_coarse"].items()}, {k: f(v) for k, v in c["p_fine"].items()})
    return O.render_rays(pc, pf, f(c["ro"]), f(c["rd"]), f(c["expr"]), f(c["latent"]) if latent is None else latent, f(c["bg"]), O.NEAR,
                         O.FAR, c["n_coarse"], c["n_fine"], t_rand=f(c["t_rand"]), noise_c=f(c["noise_c"]), u=f(c["u"]),
                         noise_f=f(c["noise_f"]), lindisp=bool(c.get("lindisp", False)), mlp=smaller_mlp)


def checksum(c) -> float:
    return C.params_checksum(c["p_coarse"]) + C.params_checksum(c["p_fine"])


def autograd(c, dtype):
    """The restatement with autograd in `dtype` on case `c`: (loss, param grads coarse, fine, latent grad, smallest |ReLU input|)."""
    pc = {k: v.to(dtype).clone().requires_grad_(True) for k, v in c["p_coarse"].items()}
    pf = {k: v.to(dtype).clone().requires_grad_(True) for k, v in c["p_fine"].items()}
    lat = c["latent"].to(dtype).clone().requires_grad_(True)
    keep, rec = torch.relu, []

    def relu(v):                                   # MLP units as they are; the density ReLU (V:52) in units of the x40 head
        rec.append(float(v.detach().abs().min()) / (1.0 if v.shape[-1] in (256, 128) else 40.0))
        return keep(v)
    torch.relu = relu
    try:
        o = run_restatement(c, dtype, params=(pc, pf), latent=lat)
    finally:
        torch.relu = keep
    loss = O.train_loss(o[0], o[3], c["tgt"].to(dtype), lat)
    loss.backward()
    return loss.detach(), pc, pf, lat.grad, min(rec)


# ------------------------------------------------------------------------------------------------------------------------------
# generator: the unmodified reference
# ------------------------------------------------------------------------------------------------------------------------------
def ref_model(ref, params):
    m = ref.models.ConditionalBlendshapePaperSmallerNeRFModel(**SMALLER_KW)
    assert list(m.state_dict().keys()) == SMALLER_KEYS and sum(v.numel() for v in m.parameters()) == SMALLER_NUMEL
    m.load_state_dict(params)
    return m


def run_reference(ref, c, grad=False):
    """ref.run_one_iter_of_nerf with this class on case `c` (oracle/make_golden.py run_reference for this family)."""
    from oracle import make_golden as MG
    from oracle import ref_import as RI
    mc, mf = ref_model(ref, c["p_coarse"]), ref_model(ref, c["p_fine"]) if c["n_fine"] > 0 else None
    opt = MG.ref_options(ref, c["n_coarse"], c["n_fine"], bool(c["stochastic"]), c["noise_std"], bool(c.get("lindisp", False)))
    enc_xyz = ref.get_embedding_function(num_encoding_functions=10, include_input=True, log_sampling=True)
    enc_dir = ref.get_embedding_function(num_encoding_functions=4, include_input=False, log_sampling=True)
    rands, randns = [], []
    if c["stochastic"]:
        rands.append(c["t_rand"])
        if c["noise_std"] > 0:
            randns.append(c["noise_c_unit"])
        if c["n_fine"] > 0:
            rands.append(c["u"])
            if c["noise_std"] > 0:
                randns.append(c["noise_f_unit"])
    latent = c["latent"].clone().requires_grad_(grad)
    ctx = torch.enable_grad() if grad else torch.no_grad()
    with ctx, RI.injected_random(rands, randns), RI.relu_clone_shim(ref):
        out = ref.run_one_iter_of_nerf(512, 512, None, mc, mf, c["ro"], c["rd"], opt, mode="train", encode_position_fn=enc_xyz,
                                       encode_direction_fn=enc_dir, expressions=c["expr"], background_prior=c["bg"], latent_code=latent)
        grads = None
        if grad:
            loss = O.train_loss(out[0], out[3], c["tgt"], latent)
            loss.backward()
            grads = {"latent": latent.grad.clone(), "loss": loss.detach().clone()}
            for tag, m in (("coarse", mc), ("fine", mf)):
                for k, v in m.named_parameters():
                    assert v.grad is not None, (tag, k)                       # all 22 tensors are live
                    grads[f"{tag}.{k}"] = v.grad.clone()
    return out, grads


def reference_margins(ref, c, tol):
    """(bit equality of reference and restatement, worst |reference fp32 - float64 restatement| / gate over the gated outputs)."""
    out_ref, _ = run_reference(ref, c)
    out_re, out64 = run_restatement(c), run_restatement(c, torch.float64)
    equal = all((a is None and b is None) or torch.equal(a, b) for a, b in zip(out_ref, out_re))
    worst = max(float((a.double() - b).abs().max()) / tol[n] for n, a, b in zip(NAMES7, out_ref, out64) if a is not None)
    return equal, worst, out_ref


def worst_vs_fp64(g, pc, pf):
    rel = lambda a, b: float((a.double() - b).norm() / (b.norm() + 1e-30))
    return max(rel(g[f"{tag}.{k}"], v.grad) for tag, po in (("coarse", pc), ("fine", pf)) for k, v in po.items())


def search(ref, n_frames=300, keep=6):
    """How the seeds of SMALLER_CASES and the frame of GRAD_CASE were chosen."""
    for name in [n for n in SMALLER_CASES if n != GRAD_CASE]:
        for s in range(11, 41, 2):
            SMALLER_CASES["_probe"] = dict(SMALLER_CASES[name], seeds=(s, s + 1))
            equal, worst, _ = reference_margins(ref, build_case("_probe"), case_tol(name))
            print(f"{name}: seeds ({s}, {s + 1}): reference == restatement {equal}, worst reference fp32 vs float64 / gate {worst:.3f}", flush=True)
            if equal and worst <= 1 / 3:
                break
    ranked = []
    for f in range(n_frames):
        SMALLER_CASES["_probe"] = dict(SMALLER_CASES[GRAD_CASE], frame=f)
        ranked.append((autograd(build_case("_probe"), torch.float64)[4], f))
    ranked.sort(reverse=True)
    for margin, f in ranked[:keep]:
        SMALLER_CASES["_probe"] = dict(SMALLER_CASES[GRAD_CASE], frame=f)
        c = build_case("_probe")
        _, g = run_reference(ref, c, grad=True)
        _, pc, pf, _, _ = autograd(c, torch.float64)
        print(f"frame {f}: smallest |ReLU input| {margin:.2e}, reference fp32 vs float64 autograd: worst tensor {worst_vs_fp64(g, pc, pf):.2e}",
              flush=True)
    SMALLER_CASES.pop("_probe")


def make_cases(ref):
    for name in SMALLER_CASES:
        if name == GRAD_CASE:
            continue
        c = build_case(name)
        equal, worst, out = reference_margins(ref, c, case_tol(name))
        print(f"[{name}] reference == restatement: {equal}; worst reference fp32 vs float64 restatement / gate: {worst:.3f}")
        assert equal, "the restatement must equal the unmodified reference bit for bit"
        assert worst <= 1 / 3, "the reference's own fp32 error uses more than a third of a gate: choose other seeds / another frame (search)"
        blob = {n: a.detach().numpy() for n, a in zip(NAMES7, out) if a is not None}
        blob["params_checksum"] = np.float64(checksum(c))
        np.savez_compressed(os.path.join(GOLD, f"{name}.npz"), **blob)


def make_grads(ref):
    """Training step through the reference (autograd, Q9 shim, the loss of O.train_loss): loss, latent gradient, the seven outputs, and
    per-tensor gradient norms / 257-element heads (full tensors of two 496,132-parameter models would exceed the size limit of a
    committed file; the MLP-level float64 comparison of tests/test_gpu_smaller.py carries the full-tensor check)."""
    c = build_case(GRAD_CASE)
    out, g = run_reference(ref, c, grad=True)
    out_re = run_restatement(c)
    assert all(torch.equal(a, b) for a, b in zip(out, out_re)), "the restatement must equal the unmodified reference bit for bit"
    _, pc, pf, lat64, margin = autograd(c, torch.float64)
    worst = worst_vs_fp64(g, pc, pf)
    e_lat = float((g["latent"].double() - lat64).norm() / lat64.norm())
    print(f"[{GRAD_CASE}] loss {float(g['loss']):.6f}; smallest |ReLU input| {margin:.2e}; reference fp32 vs float64 autograd: worst tensor "
          f"{worst:.2e}, latent {e_lat:.2e}")
    assert worst < 1e-5 and e_lat < 1e-5, "this frame has a ReLU decision within fp32 rounding: pick another (search)"
    blob = {"loss": g["loss"].numpy(), "latent": g["latent"].numpy(), "relu_margin_fp64": np.float64(margin),
            "params_checksum": np.float64(checksum(c))}
    for n, a in zip(NAMES7, out):
        blob[n] = a.detach().numpy()
    for k, v in g.items():
        if k in ("loss", "latent"):
            continue
        blob["norm:" + k] = np.float64(v.double().norm())
        blob["head:" + k] = v.reshape(-1)[:257].numpy()
    np.savez_compressed(os.path.join(GOLD, f"{GRAD_CASE}_grads.npz"), **blob)


def main():
    from oracle import ref_import as RI
    torch.set_num_threads(8)
    ref = RI.import_reference()
    if sys.argv[1:2] == ["search"]:
        search(ref)
        return
    make_cases(ref)
    make_grads(ref)


if __name__ == "__main__":
    main()

"""The two blendshape classes without a learnable code (reference nerf/models.py: ConditionalBlendshapeNeRFModel M:872-976 = "bshape",
ConditionalCompressedBlendshapeNeRFModel M:750-868 = "cbshape"): their restatements, their seeded cases, and the generator of
tests/golden/bshape_*.npz / cbshape_*.npz.  TEST INFRASTRUCTURE ONLY.

Regenerate the fixtures where the unmodified reference can be imported (oracle/ref_import.py):   python -m tests.blendshape_ref
The fixtures hold reference OUTPUTS (arrays only); inputs and weights are regenerated from seeds, a weight checksum detects drift.
`python -m tests.blendshape_ref search` prints how the seeds and frames below were chosen.
"""
from __future__ import annotations

import math
import os
import sys
from typing import Dict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import cases as C                      # noqa: E402
from oracle import nerface_oracle as O             # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAMES7 = ["rgb_c", "disp_c", "acc_c", "rgb_f", "disp_f", "acc_f", "w_last"]
KINDS = ("bshape", "cbshape")
CLASS = {"bshape": "ConditionalBlendshapeNeRFModel", "cbshape": "ConditionalCompressedBlendshapeNeRFModel"}

ENC_SHAPES = {"layers_expr.0.weight": (38, 76), "layers_expr.1.weight": (20, 38), "layers_expr.2.weight": (20, 20)}
SHAPES = {
    "bshape": dict(O.LCODE_SHAPES, **{"layer1.weight": (256, 139)}),
    "cbshape": dict(ENC_SHAPES, **dict(O.LCODE_SHAPES, **{"layer1.weight": (256, 83)})),
}
KEYS = {k: [n.replace("weight", p) for n in SHAPES[k] for p in ("weight", "bias")] for k in KINDS}          # state_dict order
NUMEL = {k: sum(s[0] * s[1] + s[0] for s in SHAPES[k].values()) for k in KINDS}                             # 335,620 / 325,410
# the trainer's keyword set (oracle.make_golden.DROPIN_MODEL_KW; neither class takes latent_code_dim)
MODEL_KW = dict(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=False, use_viewdirs=True,
                num_layers=4, hidden_size=256, include_expression=True)


def init_params(kind: str, seed: int, dtype=torch.float32, boost=True) -> Dict[str, torch.Tensor]:
    """Seeded like O.init_lcode_params: nn.Linear-style uniform init from an own generator; boost="survey": SURVEY 8(d)'s density head
    (fc_alpha.weight x40, bias 0.5), boost=True: the hard head (x300, bias 5); fc_rgb.weight x10 in both."""
    g = torch.Generator().manual_seed(seed)
    out: Dict[str, torch.Tensor] = {}
    for k, shp in SHAPES[kind].items():
        bound = 1.0 / math.sqrt(shp[1])
        out[k] = ((torch.rand(shp, generator=g, dtype=torch.float64) * 2 - 1) * bound).to(dtype)
        out[k.replace("weight", "bias")] = ((torch.rand(shp[0], generator=g, dtype=torch.float64) * 2 - 1) * bound).to(dtype)
    scale, bias = (40.0, 0.5) if boost == "survey" else (300.0, 5.0)
    if boost:
        out["fc_alpha.weight"] = out["fc_alpha.weight"] * scale
        out["fc_alpha.bias"] = torch.full_like(out["fc_alpha.bias"], bias)
        out["fc_rgb.weight"] = out["fc_rgb.weight"] * 10.0
    return out


def encoder(p, expr, acts=None):
    """layers_expr of the compressed class (M:832-834): the raw expression, a ReLU after each of the three layers."""
    e = expr.reshape(1, -1)
    for i in range(3):
        e = torch.relu(O._lin(e, p, f"layers_expr.{i}"))
        if acts is not None:
            acts.append(e)
    return e


def bshape_mlp(p, x87, expr, latent=None, masks=None, acts=None):
    """ConditionalBlendshapeNeRFModel.forward (M:935-976): the second family's network on [xyz | expr*1/3] -- O.lcode_mlp with an
    empty latent code (the class ignores the one it is handed)."""
    return O.lcode_mlp(p, x87, expr, expr.new_zeros(0), masks=masks, acts=acts)


def cbshape_mlp(p, x87, expr, latent=None, masks=None, acts=None, enc_acts=None):
    """ConditionalCompressedBlendshapeNeRFModel.forward (M:821-868): x = layer1([xyz | e3]) (no activation), then O.lcode_mlp's trunk.
    `masks` / `acts`: the trunk's hooks as in O.lcode_mlp; enc_acts collects e1, e2, e3."""
    n = x87.shape[0]
    xyz, dirs = x87[:, :63], x87[:, 63:]
    e3 = encoder(p, expr, enc_acts).repeat(n, 1)
    k = [0]

    def act(v):
        out = torch.relu(v) if masks is None else v * masks[k[0]].to(v.dtype)
        k[0] += 1
        if acts is not None:
            acts.append(out)
        return out

    x = O._lin(torch.cat((xyz, e3), dim=1), p, "layer1")
    if acts is not None:
        acts.append(x)
    for i in range(3):
        x = act(O._lin(x, p, f"layers_xyz.{i}"))
    feat = act(O._lin(x, p, "fc_feat"))
    alpha = O._lin(x, p, "fc_alpha")
    h = act(O._lin(torch.cat((feat, dirs), dim=-1), p, "layers_dir.0"))
    return torch.cat((O._lin(h, p, "fc_rgb"), alpha), dim=-1)


MLP = {"bshape": bshape_mlp, "cbshape": cbshape_mlp}

# ---- gates, copied (not imported: GPU test modules): tests/test_gpu_lcode.py TOL for the hard head (the geometry of its golden case),
# tests/smaller_ref.py TOL_SOFT for the survey head
TOL = dict(rgb_c=3e-6, rgb_f=5e-4, acc_c=1e-5, acc_f=1e-5, w_last=5e-4, disp_c=1e-5, disp_f=2e-3)          # hard head
TOL_SOFT = dict(rgb_c=3e-6, rgb_f=2e-5, acc_c=1e-5, acc_f=1e-5, w_last=1e-5, disp_c=2e-5, disp_f=2e-5)     # survey head

# name: ray / sample geometry as oracle/cases.py's case `base`, on `frame`, with weights init_params(kind, seeds[0 | 1], boost).
# Seeds and frames: the first of the scanned candidates (`search`) on which the reference's own fp32 result lies within a third of
# every output's gate of the float64 restatement -- so that a product within fp32 rounding of the exact result passes the gate.
BASES = dict(soft_eval_det_64_128=dict(frame=3, boost="survey"), soft_train_rand_64_64=dict(frame=17, boost="survey"),
             ragged_5_7=dict(frame=5, boost=True), coarse_only=dict(frame=8, boost=True))
SEEDS = {
    "bshape_soft_eval_det_64_128": (11, 12), "bshape_soft_train_rand_64_64": (11, 12), "bshape_ragged_5_7": (11, 12),
    "bshape_coarse_only": (11, 12),
    "cbshape_soft_eval_det_64_128": (17, 18), "cbshape_soft_train_rand_64_64": (17, 18), "cbshape_ragged_5_7": (17, 18),
    "cbshape_coarse_only": (11, 12),
}
CASES = {f"{kind}_{base}": dict(kind=kind, base=base, seeds=SEEDS[f"{kind}_{base}"], **spec) for kind in KINDS for base, spec in BASES.items()}
# the end-to-end GRADIENT cases: few rays, soft head, a frame without a ReLU decision within fp32 rounding -- the encoder's three
# layers included; for cbshape every encoder layer has active and inactive units on that frame.  `search` ranks frames 0..299 by
# their smallest |ReLU input| in float64 and takes the first on which the reference's fp32 autograd equals the float64 autograd to 1e-5
# in every tensor: bshape frame 208 (the first candidate: 9.0e-7, 3.0e-6), cbshape frame 164 (the eighth: 3.6e-7, 6.3e-6; 30 % .. 63 % of
# the units of an encoder layer active)
GRAD_BASE = "soft_train_noflip_64_64"
GRAD_FRAMES = {"bshape": 208, "cbshape": 164}
GRAD_CASES = {kind: f"{kind}_{GRAD_BASE}" for kind in KINDS}
for _kind in KINDS:
    CASES[GRAD_CASES[_kind]] = dict(kind=_kind, base=GRAD_BASE, frame=GRAD_FRAMES[_kind], seeds=(13, 14), boost="survey")


def case_tol(name):
    return TOL_SOFT if CASES[name]["boost"] == "survey" else TOL


def build_case(name, dtype=torch.float32, **override):
    """oracle/cases.py build_case for these classes: the geometry of CASES[name]["base"] on this case's frame and weights."""
    spec = dict(CASES[name], **override)
    c = dict(C.CASES[spec["base"]], frame=spec["frame"], kind=spec["kind"])
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
    c["p_coarse"] = init_params(spec["kind"], spec["seeds"][0], dtype, boost=spec["boost"])
    c["p_fine"] = init_params(spec["kind"], spec["seeds"][1], dtype, boost=spec["boost"])
    return c


def run_restatement(c, dtype=None, params=None):
    """O.render_rays with the class's MLP on case `c` (dtype: evaluate everything in that type)."""
    f = (lambda t: t) if dtype is None else (lambda t: None if t is None else t.to(dtype))
    pc, pf = params if params is not None else ({k: f(v) for k, v in c["p_coarse"].items()}, {k: f(v) for k, v in c["p_fine"].items()})
    return O.render_rays(pc, pf, f(c["ro"]), f(c["rd"]), f(c["expr"]), f(c["latent"]), f(c["bg"]), O.NEAR, O.FAR, c["n_coarse"],
                         c["n_fine"], t_rand=f(c["t_rand"]), noise_c=f(c["noise_c"]), u=f(c["u"]), noise_f=f(c["noise_f"]),
                         lindisp=bool(c.get("lindisp", False)), mlp=MLP[c["kind"]])


def checksum(c) -> float:
    return C.params_checksum(c["p_coarse"]) + C.params_checksum(c["p_fine"])


def autograd(c, dtype):
    """The restatement with autograd in `dtype` on case `c`: (loss, param grads coarse, fine, latent grad, smallest |ReLU input|,
    (fewest, most) active units over the encoder layers of both models, as fractions; (0, 1) for bshape)."""
    pc = {k: v.to(dtype).clone().requires_grad_(True) for k, v in c["p_coarse"].items()}
    pf = {k: v.to(dtype).clone().requires_grad_(True) for k, v in c["p_fine"].items()}
    lat = c["latent"].to(dtype).clone().requires_grad_(True)
    keep, rec, enc = torch.relu, [], []

    def relu(v):                                   # MLP units as they are; the density ReLU (V:52) in units of the x40 head
        rec.append(float(v.detach().abs().min()) / (1.0 if v.shape[-1] in (256, 128, 38, 20) else 40.0))
        if v.shape[-1] in (38, 20):
            enc.append(float((v.detach() > 0).double().mean()))
        return keep(v)
    torch.relu = relu
    try:
        o = run_restatement(c, dtype, params=(pc, pf))
    finally:
        torch.relu = keep
    loss = O.train_loss(o[0], o[3], c["tgt"].to(dtype), lat)
    loss.backward()
    return loss.detach(), pc, pf, lat.grad, min(rec), ((min(enc), max(enc)) if enc else (0.0, 1.0))


# ------------------------------------------------------------------------------------------------------------------------------
# generator: the unmodified reference
# ------------------------------------------------------------------------------------------------------------------------------
def ref_model(ref, kind, params):
    m = getattr(ref.models, CLASS[kind])(**MODEL_KW)
    assert list(m.state_dict().keys()) == KEYS[kind] and sum(v.numel() for v in m.parameters()) == NUMEL[kind]
    assert [tuple(v.shape) for k, v in m.state_dict().items() if k.endswith("weight")] == list(SHAPES[kind].values())
    m.load_state_dict(params)
    return m


def run_reference(ref, c, grad=False):
    """ref.run_one_iter_of_nerf with the class on case `c` (oracle/make_golden.py run_reference for these classes)."""
    from oracle import make_golden as MG
    from oracle import ref_import as RI
    mc = ref_model(ref, c["kind"], c["p_coarse"])
    mf = ref_model(ref, c["kind"], c["p_fine"]) if c["n_fine"] > 0 else None
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
                                       encode_direction_fn=enc_dir, expressions=c["expr"], background_prior=c["bg"],
                                       latent_code=latent if c["kind"] == "cbshape" else None)      # M:935 has no positional slot for it
        grads = None
        if grad:
            loss = O.train_loss(out[0], out[3], c["tgt"], latent)
            loss.backward()
            grads = {"latent": latent.grad.clone(), "loss": loss.detach().clone()}
            for tag, m in (("coarse", mc), ("fine", mf)):
                for k, v in m.named_parameters():
                    assert v.grad is not None, (tag, k)                       # every tensor is live
                    grads[f"{tag}.{k}"] = v.grad.clone()
    return out, grads


def reference_margins(ref, c, tol):
    """(largest |reference - fp32 restatement|, worst |reference fp32 - float64 restatement| / gate over the gated outputs)."""
    out_ref, _ = run_reference(ref, c)
    out_re, out64 = run_restatement(c), run_restatement(c, torch.float64)
    diff = max(float((a - b).abs().max()) for a, b in zip(out_ref, out_re) if a is not None)
    worst = max(float((a.double() - b).abs().max()) / tol[n] for n, a, b in zip(NAMES7, out_ref, out64) if a is not None)
    return diff, worst, out_ref


def worst_vs_fp64(g, pc, pf):
    rel = lambda a, b: float((a.double() - b).norm() / (b.norm() + 1e-30))
    return max(rel(g[f"{tag}.{k}"], v.grad) for tag, po in (("coarse", pc), ("fine", pf)) for k, v in po.items())


def search(ref, n_frames=300, keep=8):
    """How the seeds of CASES and the frames of the gradient cases were chosen."""
    for name in [n for n in CASES if n not in GRAD_CASES.values()]:
        for s in range(11, 41, 2):
            CASES["_probe"] = dict(CASES[name], seeds=(s, s + 1))
            diff, worst, _ = reference_margins(ref, build_case("_probe"), case_tol(name))
            print(f"{name}: seeds ({s}, {s + 1}): |reference - restatement| {diff:.2e}, worst reference fp32 vs float64 / gate {worst:.3f}",
                  flush=True)
            if worst <= 1 / 3:
                break
    for kind in KINDS:
        ranked = []
        for f in range(n_frames):
            CASES["_probe"] = dict(CASES[GRAD_CASES[kind]], frame=f)
            _, _, _, _, margin, (lo, hi) = autograd(build_case("_probe"), torch.float64)
            if kind == "bshape" or (lo > 0.0 and hi < 1.0):       # cbshape: an active and an inactive unit in every encoder layer
                ranked.append((margin, f))
        ranked.sort(reverse=True)
        for margin, f in ranked[:keep]:
            CASES["_probe"] = dict(CASES[GRAD_CASES[kind]], frame=f)
            c = build_case("_probe")
            _, g = run_reference(ref, c, grad=True)
            _, pc, pf, _, _, act = autograd(c, torch.float64)
            print(f"{kind} frame {f}: smallest |ReLU input| {margin:.2e}, encoder units active {act[0]:.2f} .. {act[1]:.2f}, reference fp32 "
                  f"vs float64 autograd: worst tensor {worst_vs_fp64(g, pc, pf):.2e}", flush=True)
    CASES.pop("_probe")


def make_cases(ref):
    for name in CASES:
        if name in GRAD_CASES.values():
            continue
        c = build_case(name)
        diff, worst, out = reference_margins(ref, c, case_tol(name))
        print(f"[{name}] |reference - restatement| {diff:.2e}; worst reference fp32 vs float64 restatement / gate: {worst:.3f}")
        assert worst <= 1 / 3, "the reference's own fp32 error uses more than a third of a gate: choose other seeds / another frame (search)"
        blob = {n: a.detach().numpy() for n, a in zip(NAMES7, out) if a is not None}
        blob["params_checksum"] = np.float64(checksum(c))
        np.savez_compressed(os.path.join(GOLD, f"{name}.npz"), **blob)


FULL_TENSOR_LIMIT = 4096          # gradient tensors up to this many elements are stored whole (all six encoder tensors, every bias)


def make_grads(ref, kind):
    """Training step through the reference (autograd, Q9 shim, the loss of O.train_loss): loss, latent gradient, the seven outputs, and
    the gradients of every tensor of both models -- whole where a tensor has at most FULL_TENSOR_LIMIT elements, else its norm and a
    257-element head (whole tensors of two ~330,000-parameter models would exceed the size limit of a committed file, as in
    tests/smaller_ref.py; the MLP-level float64 comparison of tests/test_gpu_blendshape.py carries the full-tensor check)."""
    name = GRAD_CASES[kind]
    c = build_case(name)
    out, g = run_reference(ref, c, grad=True)
    _, pc, pf, lat64, margin, act = autograd(c, torch.float64)
    worst = worst_vs_fp64(g, pc, pf)
    e_lat = float((g["latent"].double() - lat64).norm() / lat64.norm())
    print(f"[{name}] loss {float(g['loss']):.6f}; smallest |ReLU input| {margin:.2e}; encoder units active {act[0]:.2f} .. {act[1]:.2f}; "
          f"reference fp32 vs float64 autograd: worst tensor {worst:.2e}, latent {e_lat:.2e}")
    assert worst < 1e-5 and e_lat < 1e-5, "this frame has a ReLU decision within fp32 rounding: pick another (search)"
    assert kind == "bshape" or (act[0] > 0.0 and act[1] < 1.0), "an encoder layer is all on or all off on this frame: pick another (search)"
    blob = {"loss": g["loss"].numpy(), "latent": g["latent"].numpy(), "relu_margin_fp64": np.float64(margin),
            "params_checksum": np.float64(checksum(c))}
    for n, a in zip(NAMES7, out):
        blob[n] = a.detach().numpy()
    for k, v in g.items():
        if k in ("loss", "latent"):
            continue
        blob["norm:" + k] = np.float64(v.double().norm())
        if v.numel() <= FULL_TENSOR_LIMIT:
            blob["full:" + k] = v.numpy()
        else:
            blob["head:" + k] = v.reshape(-1)[:257].numpy()
    np.savez_compressed(os.path.join(GOLD, f"{name}_grads.npz"), **blob)


def main():
    from oracle import ref_import as RI
    torch.set_num_threads(8)
    ref = RI.import_reference()
    if sys.argv[1:2] == ["search"]:
        search(ref)
        return
    make_cases(ref)
    for kind in KINDS:
        make_grads(ref, kind)


if __name__ == "__main__":
    main()

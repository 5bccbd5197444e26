"""GPU: nerf.GraphedTrainer in every configuration it can run -- every model family in every training arithmetic, capture from a
running state (in place and through a checkpoint written by the host-stepped loop), the launcher's loop without --graph, eager
work between replays (validation renders, direct forwards, random draws) and the config switches of the iteration body.

One gate throughout: torch.equal.  The eager loop and the graph run the same kernels in the same order on the same inputs, and no
kernel of the step accumulates with floating-point atomics, so there is no tolerance to choose; the eager side is held to the float64
oracle and the reference's autograd elsewhere (test_training_trajectory_follows_oracle, the *_train_step_vs_reference_gradients
tests).  Sizes are those of tests/test_gpu_graph_trainer.py: 32 x 32 frames, 64 rays, 8 + 8 samples, 3 frames."""
import copy

import pytest
import torch

from tests.test_gpu_graph_trainer import (DECAY_FACTOR, DECAY_STEPS, FRAME_ORDER, INTRINSICS, LCODE, LR0, N_RAYS, PAPER, SIZE, _Run)

pytestmark = pytest.mark.gpu

SMALLER = "ConditionalBlendshapePaperSmallerNeRFModel"
BSHAPE, CBSHAPE = "ConditionalBlendshapeNeRFModel", "ConditionalCompressedBlendshapeNeRFModel"
NO_CODE = (BSHAPE, CBSHAPE)             # the latent row of these two moves by its regulariser gradient only: start it away from zero
SEED = 123


@pytest.fixture(autouse=True)
def _f32_afterwards():
    import nerf
    yield
    nerf.set_mlp_precision("f32")


def _run_kw(model_type):
    return dict(latent_std=0.1) if model_type in NO_CODE else {}


def _assert_state_equal(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (where, i, float((a - b).abs().max()))


_EAGER = {}


def _eager_five(gpu, model_type, precision):
    """5 steps of the eager loop body with the capturable optimizer, frames FRAME_ORDER, generator seeded with SEED: per step the
    loss terms and the snapshot; which tensors of the snapshot's parameter part received a gradient.  Computed once per combination
    and shared (nothing writes into it)."""
    import nerf
    key = (model_type, precision)
    if key not in _EAGER:
        nerf.set_mlp_precision(precision)
        run = _Run(gpu, model_type, **_run_kw(model_type))
        params = [p for g in run.opt.param_groups for p in g["params"]]
        torch.manual_seed(SEED)
        steps = []
        for k in FRAME_ORDER:
            parts = run.eager_step(k)
            steps.append((parts, run.snapshot()))
        _EAGER[key] = dict(steps=steps, stepped=[len(run.opt.state.get(p) or {}) > 0 for p in params])
    return _EAGER[key]


# ------------------------------------------------------------------------------------------ 1. every family in every arithmetic
COMBINATIONS = ([(PAPER, "bf16x3"), (LCODE, "f16x3"), (LCODE, "bf16x3"), (SMALLER, "f32")]
                + [(m, p) for m in NO_CODE for p in ("f32", "f16x3", "bf16x3")])


@pytest.mark.parametrize("model_type,precision", COMBINATIONS)
def test_graphed_steps_equal_eager_steps_in_every_family_and_arithmetic(hip_lib, gpu, model_type, precision):
    """The body of test_graphed_steps_equal_eager_steps for the ten combinations it leaves out: 5 steps, frames [0, 2, 1, 1, 0];
    parameters, latent table, background, both Adam moments and parts[:7] are torch.equal after every step.  Then: every tensor that
    received a gradient in the eager run has left its initial value in the GRAPHED run (equality cannot hold because nothing moved) --
    for the compressed blendshape class that includes the six layers_expr tensors of either model, which only the condition kernel's
    gradient scatter reaches -- and check_range() passes."""
    import nerf
    nerf.set_mlp_precision(precision)
    want = _eager_five(gpu, model_type, precision)
    graphed = _Run(gpu, model_type, **_run_kw(model_type))
    params = [p for g in graphed.opt.param_groups for p in g["params"]]
    initial = [p.detach().clone() for p in params]
    if model_type in NO_CODE:
        assert all(float(row.abs().max()) > 0 for row in graphed.latent.detach())
    torch.manual_seed(SEED)
    tr = graphed.trainer(precision)
    for step, k in enumerate(FRAME_ORDER):
        parts = graphed.graph_step(tr, k)
        assert torch.equal(parts[:7], want["steps"][step][0][:7]), (step, parts, want["steps"][step][0])
        _assert_state_equal(graphed.snapshot(), want["steps"][step][1], step)
    assert bool(torch.isfinite(tr.parts[:7]).all())
    assert float(graphed.opt.state[graphed.latent]["step"]) == 5.0
    stepped = want["stepped"]
    assert sum(stepped) >= len(stepped) - 5                               # all but the background and the paper model's dead layers_dir.3
    for i, (p, p0, s) in enumerate(zip(params, initial, stepped)):
        assert torch.equal(p.detach(), p0) != s, (i, s, "a tensor with a gradient did not move / one without did")
    ids = [id(p) for p in params]
    assert stepped[ids.index(id(graphed.latent))]
    if model_type == CBSHAPE:
        named = [(n, p) for m in (graphed.model_c, graphed.model_f) for n, p in m.named_parameters() if n.startswith("layers_expr")]
        assert len(named) == 12
        for n, p in named:
            assert stepped[ids.index(id(p))] and not torch.equal(p.detach(), initial[ids.index(id(p))]), n
    tr.check_range()


def test_smaller_model_refuses_split_fp16_under_capture_and_trains_in_f32_afterwards(hip_lib, gpu):
    """The smaller paper model has exact-f32 kernels only: a trainer built for "f16x3" raises NotImplementedError from its first
    step (before a parameter is touched), and an "f32" trainer on the same models then runs the eager loop's steps."""
    want = _eager_five(gpu, SMALLER, "f32")
    graphed = _Run(gpu, SMALLER)
    before = graphed.snapshot()
    tr = graphed.trainer("f16x3")
    with pytest.raises(NotImplementedError, match="f16x3"):
        graphed.graph_step(tr, 0)
    _assert_state_equal(graphed.snapshot(), before, "after the refusal")
    import nerf
    assert nerf.get_mlp_precision() == "f32"
    torch.manual_seed(SEED)
    tr = graphed.trainer("f32")
    for step, k in enumerate(FRAME_ORDER[:2]):
        parts = graphed.graph_step(tr, k)
        assert torch.equal(parts[:7], want["steps"][step][0][:7])
        _assert_state_equal(graphed.snapshot(), want["steps"][step][1], step)


# ------------------------------------------------------------------------------------------ 2. capture from a running state
@pytest.mark.parametrize("model_type,precision", [(PAPER, "f32"), (LCODE, "bf16x3")])
def test_capture_after_eager_steps_resumes_in_place(hip_lib, gpu, model_type, precision):
    """2 eager steps on the twin with the capturable optimizer, then the trainer is built and takes 3 replays: the capture's undo has
    moments and a running state block to RESTORE (its copy_ branches), and the state after each replay equals steps 3-5 of the 5-step
    eager run."""
    import nerf
    nerf.set_mlp_precision(precision)
    want = _eager_five(gpu, model_type, precision)
    graphed = _Run(gpu, model_type)
    torch.manual_seed(SEED)
    for step, k in enumerate(FRAME_ORDER[:2]):
        graphed.eager_step(k)
        _assert_state_equal(graphed.snapshot(), want["steps"][step][1], step)
    tr = graphed.trainer(precision)
    for step, k in list(enumerate(FRAME_ORDER))[2:]:
        parts = graphed.graph_step(tr, k)
        assert torch.equal(parts[:7], want["steps"][step][0][:7]), (step, parts, want["steps"][step][0])
        _assert_state_equal(graphed.snapshot(), want["steps"][step][1], step)
    assert all(float(graphed.opt.state[p]["step"]) == 5.0 for p in graphed.opt.state)
    tr.check_range()


_HOST = {}


def _host_loop_five(gpu):
    """5 steps of the loop users run without --graph (paper model, f32): the default, host-stepped nerf.optim.Adam, zero_grad(), `lr`
    rewritten on the host after every step.  Also what a checkpoint after step 2 holds, and the generator's state at that point."""
    if not _HOST:
        run = _Run(gpu, PAPER, capturable=False)
        torch.manual_seed(SEED)
        steps = []
        for i, k in enumerate(FRAME_ORDER):
            parts = run.eager_step(k)
            steps.append((parts, run.snapshot()))
            if i == 1:
                clone = lambda sd: {n: v.detach().clone() for n, v in sd.items()}
                _HOST["checkpoint"] = dict(model_coarse_state_dict=clone(run.model_c.state_dict()),
                                           model_fine_state_dict=clone(run.model_f.state_dict()),
                                           latent_codes=run.latent.detach().clone(), background=run.background.detach().clone(),
                                           optimizer_state_dict=copy.deepcopy(run.opt.state_dict()))
                _HOST["rng"] = torch.cuda.get_rng_state(gpu)
        assert all(float(st["step"]) == 5.0 and not st["step"].is_cuda for st in run.opt.state.values())
        _HOST["steps"] = steps
        _HOST["lr"] = [g["lr"] for g in run.opt.state_dict()["param_groups"]]
    return _HOST


def test_graphed_run_equals_the_launchers_host_stepped_loop(hip_lib, gpu):
    """5 replays against the launcher's loop without --graph from step 0: the device-side step count and rate against
    nf_adam_step fed `lr` from the host expression (bit-equal for steps 0-19 of this schedule, as
    test_replays_touch_only_the_frames_row_and_train shows on hardware)."""
    want = _host_loop_five(gpu)
    graphed = _Run(gpu, PAPER)
    torch.manual_seed(SEED)
    tr = graphed.trainer("f32")
    for step, k in enumerate(FRAME_ORDER):
        parts = graphed.graph_step(tr, k)
        assert torch.equal(parts[:7], want["steps"][step][0][:7]), (step, parts, want["steps"][step][0])
        _assert_state_equal(graphed.snapshot(), want["steps"][step][1], step)
    assert [g["lr"] for g in graphed.opt.state_dict()["param_groups"]] == want["lr"]


def test_capture_after_a_checkpoint_of_the_host_stepped_loop(hip_lib, gpu):
    """eager -> graph through a checkpoint, crossing optimizer kinds: the state_dicts the host-stepped loop holds after 2 steps are
    loaded into a fresh twin with nerf.optim.Adam(capturable=True) + set_lr_schedule, as launch/train_sharded.py --load-checkpoint
    ... --graph does; 3 replays equal steps 3-5 of the loop that wrote the checkpoint, moments (from optimizer.state on both sides)
    and reported `lr` included."""
    want = _host_loop_five(gpu)
    ck = want["checkpoint"]
    graphed = _Run(gpu, PAPER)
    graphed.model_c.load_state_dict(ck["model_coarse_state_dict"])
    graphed.model_f.load_state_dict(ck["model_fine_state_dict"])
    with torch.no_grad():
        graphed.latent.copy_(ck["latent_codes"])
        graphed.background.copy_(ck["background"])
    graphed.opt.load_state_dict(copy.deepcopy(ck["optimizer_state_dict"]))
    graphed.opt.set_lr_schedule(LR0, DECAY_FACTOR, DECAY_STEPS)
    _assert_state_equal(graphed.snapshot(), want["steps"][1][1], "loaded")
    torch.cuda.set_rng_state(want["rng"], gpu)                            # the draws continue where the checkpointed loop's did
    tr = graphed.trainer("f32")
    for step, k in list(enumerate(FRAME_ORDER))[2:]:
        parts = graphed.graph_step(tr, k)
        assert torch.equal(parts[:7], want["steps"][step][0][:7]), (step, parts, want["steps"][step][0])
        _assert_state_equal(graphed.snapshot(), want["steps"][step][1], step)
    assert all(float(graphed.opt.state[p]["step"]) == 5.0 for p in graphed.opt.state)
    sd = graphed.opt.state_dict()
    assert [g["lr"] for g in sd["param_groups"]] == want["lr"]
    assert all(float(st["step"]) == 5.0 and not st["step"].is_cuda for st in sd["state"].values())


# ------------------------------------------------------------------------------------------ 3. eager work between replays
def _direct_forward(run, k, x87):
    """model(x87, expr, latent) on pre-encoded points: through the version-keyed weight cache, without a pack-epoch bump."""
    with torch.no_grad():
        return run.model_c(x87, run.exprs[k], torch.zeros(32, device=x87.device)).clone()


def _validation_render(run, k):
    """The launcher's validation block on frame k: eval(), no_grad, a whole 32 x 32 frame in `validation` mode (which perturbs the
    depths: random draws from the generator the replays draw from), a zero latent code, the frame's expression."""
    import nerf
    run.model_c.eval(), run.model_f.eval()
    with torch.no_grad():
        ro, rd = nerf.get_ray_bundle(SIZE, SIZE, INTRINSICS, run.poses[k])
        out = nerf.run_one_iter_of_nerf(SIZE, SIZE, INTRINSICS, run.model_c, run.model_f, ro, rd, run.cfg, mode="validation",
                                        encode_position_fn=run.enc[0], encode_direction_fn=run.enc[1], expressions=run.exprs[k],
                                        background_prior=run.background.view(-1, 3), latent_code=torch.zeros(32, device=ro.device))
    run.model_c.train(), run.model_f.train()
    assert len(out) == 7 and all(o is not None for o in out)
    return [o.clone() for o in out]


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_validation_renders_and_direct_forwards_between_replays(hip_lib, gpu, precision):
    """Two twins from one seed, 5 steps; after steps 2 and 4 both render a validation frame and then call the coarse model directly
    on 100 encoded points; the direct call is also made right after steps 1, 3 and 5, where no render has re-packed the weights since
    the last step, so that only the version counters (GraphedTrainer.step's increment_version loop on the graphed side) can tell the
    cache that the replay wrote the parameters.  Outputs of every render and direct call, and the training state after every step,
    are torch.equal between the twins: eager draws between replays leave the replayed draws in step with the eager loop."""
    import nerf
    nerf.set_mlp_precision(precision)
    g = torch.Generator().manual_seed(17)
    pts, dirs = (0.2 * torch.randn(100, 3, generator=g)).to(gpu), torch.nn.functional.normalize(torch.randn(100, 3, generator=g)).to(gpu)
    val_cfg = dict(num_coarse=8, num_fine=8)

    def drive(run, step_fn):
        x87 = torch.cat((run.enc[0](pts), run.enc[1](dirs)), dim=-1)
        assert x87.shape == (100, 87)
        torch.manual_seed(SEED)
        log = []
        for step, k in enumerate(FRAME_ORDER):
            parts = step_fn(k)
            entry = dict(parts=parts, state=run.snapshot(), render=None)
            if step in (1, 3):
                entry["render"] = _validation_render(run, k)
            entry["direct"] = _direct_forward(run, k, x87)
            log.append(entry)
        return log

    eager = _Run(gpu, PAPER, val_cfg=val_cfg)
    assert bool(eager.cfg.nerf.validation.perturb)                        # the renders draw from the generator
    want = drive(eager, eager.eager_step)
    graphed = _Run(gpu, PAPER, val_cfg=val_cfg)
    tr = graphed.trainer(precision)
    got = drive(graphed, lambda k: graphed.graph_step(tr, k))
    for step, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a["parts"][:7], b["parts"][:7]), (step, a["parts"], b["parts"])
        _assert_state_equal(a["state"], b["state"], step)
        assert torch.equal(a["direct"], b["direct"]), (step, "direct forward", float((a["direct"] - b["direct"]).abs().max()))
        assert (a["render"] is None) == (b["render"] is None)
        if a["render"] is not None:
            _assert_state_equal(a["render"], b["render"], (step, "validation output"))
            assert a["render"][0].shape == (SIZE, SIZE, 3) and bool(torch.isfinite(a["render"][3]).all())
    assert not torch.equal(got[1]["direct"], got[3]["direct"])            # the weights the direct call saw moved
    assert not torch.equal(got[1]["render"][3], got[3]["render"][3])
    tr.check_range()


# ------------------------------------------------------------------------------------------ 4. config switches under capture
SWITCHES = {
    "two_chunks_of_32": dict(train_cfg=dict(chunksize=32)),
    "chunks_of_48_and_16": dict(train_cfg=dict(chunksize=48)),
    "no_fine_pass": dict(train_cfg=dict(num_fine=0)),
    "no_background": dict(background=False),
    "white_background": dict(train_cfg=dict(white_background=True)),
    "lindisp": dict(train_cfg=dict(lindisp=True)),
    "deterministic": dict(train_cfg=dict(perturb=False, radiance_field_noise_std=0.0)),
    "pose_4x4": dict(pose44=True),
    "supervised_background_two_chunks": dict(train_background=True, train_cfg=dict(chunksize=32)),
}
SWITCH_FRAMES = (0, 2, 1)


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_config_switches_under_capture_equal_eager(hip_lib, gpu, switch):
    """One switch of the iteration body per case, paper model, f32, 3 steps, graph against an eager twin with the capturable
    optimizer: torch.equal after every step, a finite loss, and the latent row of the frame used moved."""
    kw = SWITCHES[switch]
    eager, graphed = _Run(gpu, PAPER, **kw), _Run(gpu, PAPER, **kw)
    n_chunks = -(-N_RAYS // int(eager.cfg.nerf.train.chunksize))
    assert n_chunks == {"two_chunks_of_32": 2, "chunks_of_48_and_16": 2, "supervised_background_two_chunks": 2}.get(switch, 1)
    if switch == "pose_4x4":
        assert graphed.poses[0].shape == (4, 4)
    fine0 = [p.detach().clone() for p in graphed.model_f.parameters()]
    torch.manual_seed(SEED)
    want = []
    for k in SWITCH_FRAMES:
        parts = eager.eager_step(k)
        want.append((parts, eager.snapshot()))
    torch.manual_seed(SEED)
    tr = graphed.trainer("f32")
    n_parts = 8 if kw.get("train_background") else 7
    for step, k in enumerate(SWITCH_FRAMES):
        row0 = graphed.latent[k].detach().clone()
        parts = graphed.graph_step(tr, k)
        assert torch.equal(parts[:n_parts], want[step][0][:n_parts]), (step, parts, want[step][0])
        _assert_state_equal(graphed.snapshot(), want[step][1], step)
        assert bool(torch.isfinite(parts[:n_parts]).all())
        assert not torch.equal(graphed.latent[k].detach(), row0)
    if switch == "no_fine_pass":
        assert tr.has_fine is False
        assert torch.equal(tr.parts[2], want[2][0][2]) and float(tr.parts[2]) == 0.0
        for run in (eager, graphed):
            for p, p0 in zip(run.model_f.parameters(), fine0):
                assert torch.equal(p.detach(), p0) and len(run.opt.state.get(p) or {}) == 0
            n_c = len(list(run.model_c.parameters()))                     # all of the coarse model but its dead layers_dir.3
            assert sum(len(run.opt.state.get(p) or {}) > 0 for p in run.model_c.parameters()) == n_c - 2
    else:
        assert tr.has_fine is True
    if switch == "no_background":
        assert len(graphed.opt.param_groups) == 1 and graphed.background is None
    if switch == "supervised_background_two_chunks":
        assert float(tr.parts[7]) > 0.0 and len(graphed.opt.state.get(graphed.background) or {}) > 0

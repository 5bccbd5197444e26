"""CPU: the host side of the captured training step -- nerf.optim.Adam(capturable=True)'s state layout, the device learning-rate
formula restated, and the refusals of nerf.GraphedTrainer / nerf.training_loss that need no device."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 3), (7,), (2, 2, 2))]


def _stepped_torch_adam(n_steps=3):
    ps = _params()
    opt = torch.optim.Adam([{"params": ps[:2]}, {"params": ps[2:], "lr": 2e-3}], lr=1e-3)
    for k in range(n_steps):
        for p in ps:
            p.grad = torch.full_like(p, 0.1 * (k + 1))
        opt.step()
    return ps, opt


def _same_state(sd_a, sd_b):
    assert sd_a["state"].keys() == sd_b["state"].keys()
    for k in sd_a["state"]:
        a, b = sd_a["state"][k], sd_b["state"][k]
        assert float(a["step"]) == float(b["step"])
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    assert [g["lr"] for g in sd_a["param_groups"]] == [g["lr"] for g in sd_b["param_groups"]]
    assert [g["params"] for g in sd_a["param_groups"]] == [g["params"] for g in sd_b["param_groups"]]


def test_capturable_state_dict_round_trips_with_torch_adam_and_the_default_form():
    import nerf
    ps, ref = _stepped_torch_adam(3)
    sd_ref = copy.deepcopy(ref.state_dict())
    groups = lambda: [{"params": _params()[:2]}, {"params": _params()[2:], "lr": 2e-3}]
    cap = nerf.optim.Adam(groups(), lr=1e-3, capturable=True)
    cap.load_state_dict(sd_ref)
    # inside: every step of a group is a 0-d float32 view onto that group's one block
    for gi, g in enumerate(cap.param_groups):
        for p in g["params"]:
            s = cap.state[p]["step"]
            assert s.dtype == torch.float32 and s.dim() == 0 and float(s) == 3.0
            assert s.data_ptr() == cap._blocks[gi].data_ptr()
    sd_cap = cap.state_dict()
    for st in sd_cap["state"].values():                                   # outside: torch's default layout
        assert torch.is_tensor(st["step"]) and st["step"].dtype == torch.float32 and st["step"].dim() == 0 and not st["step"].is_cuda
    _same_state(sd_cap, sd_ref)
    # -> torch.optim.Adam, which keeps stepping from it
    ps2 = _params()
    back = torch.optim.Adam([{"params": ps2[:2]}, {"params": ps2[2:], "lr": 2e-3}], lr=1e-3)
    back.load_state_dict(copy.deepcopy(sd_cap))          # torch adopts the step tensors it is handed
    _same_state(back.state_dict(), sd_ref)
    for p, q in zip(ps2, ps):
        p.data.copy_(q.data)
        p.grad = torch.full_like(p, 0.25)
        q.grad = torch.full_like(q, 0.25)
    back.step()
    ref.step()
    assert all(torch.equal(p, q) for p, q in zip(ps2, ps))
    assert all(float(st["step"]) == 4.0 for st in back.state_dict()["state"].values())
    # -> the default nerf.optim.Adam (0-d float32 CPU steps), and from it back into the capturable form
    dflt = nerf.optim.Adam(groups(), lr=1e-3)
    dflt.load_state_dict(sd_cap)
    for st in dflt.state.values():
        assert st["step"].dtype == torch.float32 and not st["step"].is_cuda and float(st["step"]) == 3.0
    _same_state(dflt.state_dict(), sd_ref)
    cap2 = nerf.optim.Adam(groups(), lr=1e-3, capturable=True)
    cap2.load_state_dict(dflt.state_dict())
    _same_state(cap2.state_dict(), sd_ref)
    # an old checkpoint holds python ints
    sd_int = ref.state_dict()
    for st in sd_int["state"].values():
        st["step"] = int(st["step"])
    cap3 = nerf.optim.Adam(groups(), lr=1e-3, capturable=True)
    cap3.load_state_dict(sd_int)
    assert all(float(st["step"]) == 4.0 and torch.is_tensor(st["step"]) for st in cap3.state_dict()["state"].values())


def test_capturable_refuses_mixed_step_counts_in_a_group_and_default_construction_is_unchanged():
    import nerf
    _, ref = _stepped_torch_adam(2)
    sd = ref.state_dict()
    sd["state"][0]["step"] = torch.tensor(5.0)
    cap = nerf.optim.Adam([{"params": _params()[:2]}, {"params": _params()[2:], "lr": 2e-3}], lr=1e-3, capturable=True)
    with pytest.raises(ValueError, match="different numbers of steps"):
        cap.load_state_dict(sd)
    dflt = nerf.optim.Adam(_params(), lr=1e-3)
    assert dflt.capturable is False and dflt._blocks == {}
    with pytest.raises(RuntimeError, match="capturable=True"):
        dflt.set_lr_schedule(1e-3, 0.1, 1000.0)


def _device_lr(step_done, lr0, factor, steps):
    """csrc/nf_optim.hip, k_adam_step_dev, restated: doubles throughout, one rounding to float32."""
    s = np.float64(np.float32(step_done))                                 # the counter is a float32
    lr = np.float64(lr0) if s == 0.0 else np.float64(lr0) * np.power(np.float64(factor), (s - 1.0) / np.float64(steps))
    return np.float32(lr)


@pytest.mark.parametrize("i", [0, 1, 999, 250000])
def test_device_lr_formula_is_the_trainers_schedule(i):
    import nerf
    lr0, factor, decay = 5.0e-4, 0.1, 250
    # what the loop of launch/train_sharded.py feeds step i: lr0 at i = 0, else the lr_new it set at the end of step i - 1
    host = lr0 if i == 0 else lr0 * (factor ** ((i - 1) / (decay * 1000)))
    got = _device_lr(i, lr0, factor, decay * 1000)
    want = np.float32(host)
    assert abs(float(got) - float(want)) <= float(np.spacing(want)), (i, got, want)
    opt = nerf.optim.Adam(_params(), lr=lr0, capturable=True)
    opt.set_lr_schedule(lr0, factor, decay * 1000)
    assert opt.scheduled_lr(float(i), lr0) == host                        # state_dict()'s `lr` is the same expression


def _world2_worker(rank, world, port, q):
    sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import nerf
        table = torch.zeros(3, 32, requires_grad=True)
        opt = nerf.optim.Adam([table], lr=1e-3, capturable=True)
        try:
            nerf.GraphedTrainer(None, None, table, None, opt, 32, 32, [48.0, 48.0, 0.5, 0.5], None, "f32")
            q.put((rank, "no error"))
        except NotImplementedError as e:
            q.put((rank, "NotImplementedError: " + str(e)))
        except Exception as e:                                            # noqa: BLE001
            q.put((rank, f"{type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()


def test_graphed_trainer_refuses_more_than_one_rank():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_world2_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [r[0] for r in res] == [0, 1]
    for _, msg in res:
        assert msg.startswith("NotImplementedError") and "single-rank" in msg and "world size 2" in msg, msg


def test_graphed_trainer_refuses_a_host_stepped_optimizer_and_unknown_precisions():
    import nerf
    table = torch.zeros(3, 32, requires_grad=True)
    with pytest.raises(TypeError, match="capturable=True"):
        nerf.GraphedTrainer(None, None, table, None, nerf.optim.Adam([table], lr=1e-3), 32, 32, None, None, "f32")
    with pytest.raises(ValueError, match="precision"):
        nerf.GraphedTrainer(None, None, table, None, nerf.optim.Adam([table], lr=1e-3, capturable=True), 32, 32, None, None, "f16x2")


def test_training_loss_background_term_needs_the_last_weight():
    import nerf
    rgb, tgt, bg = torch.rand(8, 3), torch.rand(8, 3), torch.rand(8, 3)
    with pytest.raises(ValueError, match="last_weight"):
        nerf.training_loss(rgb, None, tgt, None, background=bg)
    with pytest.raises(ValueError, match="background"):
        nerf.training_loss(rgb, None, tgt, None, last_weight=torch.rand(8))

"""Wall time and dispatches per training iteration of the NeRFace path, eager loop body against nerf.GraphedTrainer, in one process.

    python tools/time_train_step.py [--size 512] [--rays 2048] [--samples 64] [--iters 200] [--warmup 20] [--repeats 5]
                                    [--precisions f32 f16x3 bf16x3] [--markdown profiles/graph_trainer.md]

Eager = the loop body of launch/train_sharded.py as it stands without --graph (nerf.optim.Adam stepped from the host, `lr`
rewritten on the host).  Graphed = the same body replayed by nerf.GraphedTrainer (nerf.optim.Adam(capturable=True)).
Wall time: host time between two device synchronisations around --iters iterations after --warmup iterations, per iteration; the
median of --repeats such measurements, with their min and max.  Dispatches: device kernels and memsets per iteration as the torch
profiler records them over 10 iterations ("n/a" if the profiler does not see into a replayed graph).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "4d-facial-avatars_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import make_synthetic_dataset as MS  # noqa: E402
import nerf  # noqa: E402
from launch import common as CM  # noqa: E402

N_FRAMES = 8
LR0, FACTOR, DECAY = 5.0e-4, 0.1, 250


class Setup:
    def __init__(self, args, dev, capturable):
        cfgd = MS.config("unused", "unused", num_random_rays=args.rays)
        cfgd["nerf"]["train"].update(num_coarse=args.samples, num_fine=args.samples)
        self.cfg = nerf.CfgNode(cfgd)
        torch.manual_seed(0)
        self.model_c, self.model_f = CM.build_models(self.cfg, dev)
        self.model_c.train(), self.model_f.train()
        g = torch.Generator().manual_seed(1)
        s = args.size
        self.size, self.n_rays = s, args.rays
        self.intr = np.array([-1.5 * s, 1.5 * s, 0.5, 0.5])
        self.latent = torch.zeros(N_FRAMES, 32, device=dev, requires_grad=True)
        self.background = torch.rand(s, s, 3, generator=g).to(dev)
        groups = [{"params": list(self.model_c.parameters()) + list(self.model_f.parameters()) + [self.latent]},
                  {"params": self.background, "lr": LR0}]
        self.opt = nerf.optim.Adam(groups, lr=LR0, capturable=capturable)
        self.poses = [torch.tensor(MS.frame_pose(f), dtype=torch.float32)[:3, :4].contiguous().to(dev) for f in range(N_FRAMES)]
        self.exprs = [(0.5 * torch.randn(76, generator=g)).to(dev) for _ in range(N_FRAMES)]
        self.imgs = [torch.rand(s, s, 3, generator=g).to(dev) for _ in range(N_FRAMES)]
        self.maps = [(torch.rand(s * s, generator=g) + 0.1).to(dev) for _ in range(N_FRAMES)]
        self.rows = torch.arange(N_FRAMES, device=dev)
        self.enc = (nerf.get_embedding_function(10, True, True), nerf.get_embedding_function(4, False, True))
        self.i = 0
        self.trainer = None
        if capturable:
            self.opt.set_lr_schedule(LR0, FACTOR, DECAY * 1000)

    def eager(self):
        k, s = self.i % N_FRAMES, self.size
        latent = self.latent[k]
        sel = nerf.choose_rays(self.maps[k], self.n_rays)
        ro, rd, target, bg = nerf.get_ray_batch(s, s, self.intr, self.poses[k], sel, self.imgs[k], self.background)
        rgb_c, _, _, rgb_f, _, _, _ = nerf.run_one_iter_of_nerf(
            s, s, self.intr, self.model_c, self.model_f, ro, rd, self.cfg, mode="train", encode_position_fn=self.enc[0],
            encode_direction_fn=self.enc[1], expressions=self.exprs[k], background_prior=bg, latent_code=latent)
        loss, _ = nerf.training_loss(rgb_c[..., :3], rgb_f[..., :3], target[..., :3], latent)
        loss.backward()
        self.opt.step()
        self.opt.zero_grad()
        lr_new = LR0 * (FACTOR ** (self.i / (DECAY * 1000)))
        for g in self.opt.param_groups:
            g["lr"] = lr_new
        self.i += 1

    def graphed(self):
        k, s = self.i % N_FRAMES, self.size
        if self.trainer is None:
            self.trainer = nerf.GraphedTrainer(self.model_c, self.model_f, self.latent, self.background, self.opt, s, s, self.intr,
                                               self.cfg, nerf.get_mlp_precision())
        self.trainer.step(self.poses[k], self.exprs[k], self.imgs[k], self.maps[k], self.rows[k])
        self.i += 1


def wall_ms(step, iters, warmup, repeats):
    out = []
    for _ in range(repeats):
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return out


def dispatches(step, iters=10):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(iters):
                step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n / iters if n else None
    except Exception as e:                                                # noqa: BLE001
        print(f"(profiler unavailable: {type(e).__name__}: {e})")
        return None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precisions", nargs="+", default=["f32", "f16x3", "bf16x3"])
    ap.add_argument("--markdown", type=str, default="")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    rows = []
    for prec in args.precisions:
        nerf.set_mlp_precision(prec)
        res = {}
        for mode in ("eager", "graphed"):
            su = Setup(args, dev, capturable=(mode == "graphed"))
            step = getattr(su, mode)
            t = wall_ms(step, args.iters, args.warmup, args.repeats)
            res[mode] = (statistics.median(t), min(t), max(t), dispatches(step))
            print(f"{prec:7s} {mode:8s} {res[mode][0]:.3f} ms / iteration (min {res[mode][1]:.3f}, max {res[mode][2]:.3f}), "
                  f"dispatches / iteration: {res[mode][3]}", flush=True)
            del su
            torch.cuda.empty_cache()
        rows.append((prec, res))
    nerf.set_mlp_precision("f32")
    if args.markdown:
        fmt = lambda d: "n/a" if d is None else f"{d:.1f}"
        with open(args.markdown, "w") as f:
            f.write("# Training iteration: eager loop body against nerf.GraphedTrainer\n\n")
            f.write(f"Command: `python tools/time_train_step.py {' '.join(sys.argv[1:] if argv is None else argv)}`\n\n")
            f.write(f"Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; paper model pair, {args.size} x {args.size} frames, "
                    f"{args.rays} rays, {args.samples} + {args.samples} samples.\n\n")
            f.write(f"Wall time per iteration: host time between two device synchronisations around {args.iters} iterations after "
                    f"{args.warmup} warm-up iterations; median (min .. max) of {args.repeats} repeats, same process.  Dispatches: device "
                    "kernels and memsets per iteration as the torch profiler records them over 10 iterations.\n\n")
            f.write("| precision | eager ms | graphed ms | graphed / eager | eager noise (max - min) ms | eager dispatches | graphed dispatches |\n")
            f.write("|---|---|---|---|---|---|---|\n")
            for prec, r in rows:
                e, g = r["eager"], r["graphed"]
                f.write(f"| {prec} | {e[0]:.3f} ({e[1]:.3f} .. {e[2]:.3f}) | {g[0]:.3f} ({g[1]:.3f} .. {g[2]:.3f}) | {g[0] / e[0]:.3f} | "
                        f"{e[2] - e[1]:.3f} | {fmt(e[3])} | {fmt(g[3])} |\n")
            slower = [p for p, r in rows if r["graphed"][0] > r["eager"][0] + (r["eager"][2] - r["eager"][1])]
            f.write("\n" + (f"The graphed step is SLOWER than the eager step by more than the eager run-to-run spread for: {', '.join(slower)}.\n"
                            if slower else "The graphed step is not slower than the eager step beyond the eager run-to-run spread for any precision.\n"))
    return rows


if __name__ == "__main__":
    main()

"""What the image metrics cost on the GPU, against the frame they measure -- one process, HIP events, warm-up, medians.

    python tools/time_image_metrics.py [--size 512] [--frames 16] [--rounds 3] [--out FILE.json]

(a) nf_image_metrics alone at size x size, N = 1: REPS calls back to back between one event pair (the call's memset of its tickets
    included), the median of ROUNDS such windows; through nerf.image_metrics (which also allocates the workspace and the outputs)
    and through the C entry point with buffers allocated once.
(b) launch/eval_sharded.py on a synthetic sequence of that size with --precision f16x2 (the fastest arithmetic), ROUNDS times
    alternately without and with --metrics after a warm-up run of each kind: the yardstick is the median over the rounds of the
    median frame time without the flag; against it stand the median of the launch's own event pair per frame (metrics_s: test image
    upload, quantisation, the launch) and the difference of the median frame time with the flag.  Both must stay below 1 %.
    (The launcher's last_stats carries the per-frame times as "frame_s" / "metrics_frame_s" for this.)
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "4d-facial-avatars_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPS, ROUNDS = 200, 9


def window_us(fn):
    """Median over ROUNDS of (REPS calls between two events) / REPS, microseconds."""
    for _ in range(20):
        fn()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / REPS)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_image_metrics.py measures on a ROCm device; there is none")
    import yaml
    import make_synthetic_dataset as MS
    import nerf
    from nerf import _hip as H
    from launch import common as CM
    from launch import eval_sharded
    dev = torch.device("cuda:0")
    s = args.size
    res = {"device": torch.cuda.get_device_name(0), "size": s, "reps": REPS, "rounds": ROUNDS}
    # ---- (a) the kernel alone
    rng = np.random.RandomState(0)
    a = torch.from_numpy(rng.randint(0, 256, (1, s, s, 3)).astype(np.uint8)).to(dev)
    b = torch.from_numpy(rng.randint(0, 256, (1, s, s, 3)).astype(np.uint8)).to(dev)
    res["python_call_us"] = window_us(lambda: nerf.image_metrics(a, b))
    lib = H.lib()
    need = lib.nf_image_metrics_workspace_bytes(1, s, s)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    of, oi = torch.empty((1, 4), dtype=torch.float64, device=dev), torch.empty((1, 2), dtype=torch.int64, device=dev)
    st = H.stream_ptr(dev)
    res["c_call_us"] = window_us(lambda: lib.nf_image_metrics(H.ptr(a), H.ptr(b), 1, s, s, 2.0, H.ptr(ws), need, H.ptr(of), H.ptr(oi), st))
    res["bytes_read"] = 2 * s * s * 3
    # ---- (b) in the launcher, against the f16x2 frame
    with tempfile.TemporaryDirectory() as base:
        data = MS.write(os.path.join(base, "data"), size=s, n_train=1, n_val=1, n_test=args.frames)
        cfg_path = os.path.join(base, "config.yml")
        with open(cfg_path, "w") as f:
            yaml.safe_dump(MS.config(data, os.path.join(base, "logs")), f)
        torch.manual_seed(0)
        model_c, model_f = CM.build_models(CM.load_config(cfg_path), dev)
        ck = os.path.join(base, "untrained.ckpt")
        torch.save({"model_coarse_state_dict": model_c.state_dict(), "model_fine_state_dict": model_f.state_dict()}, ck)
        common = ["--config", cfg_path, "--checkpoint", ck, "--precision", "f16x2", "--verify-gate", "0"]

        def run(tag, extra):
            eval_sharded.main(common + ["--savedir", os.path.join(base, tag)] + extra)
            return dict(eval_sharded.main.last_stats)
        run("warm_plain", [])
        run("warm_metrics", ["--metrics"])
        plain, with_m = [], []
        for k in range(args.rounds):                                  # alternate: a drift of the box shows in both
            plain.append(run(f"plain{k}", []))
            with_m.append(run(f"metrics{k}", ["--metrics"]))
    med = statistics.median
    res["frames"], res["launcher_rounds"] = args.frames, args.rounds
    res["frame_f16x2_ms_per_round"] = [1e3 * med(r["frame_s"]) for r in plain]
    res["frame_f16x2_with_metrics_ms_per_round"] = [1e3 * med(r["frame_s"]) for r in with_m]
    res["frame_f16x2_ms"] = med(res["frame_f16x2_ms_per_round"])
    res["frame_f16x2_with_metrics_ms"] = med(res["frame_f16x2_with_metrics_ms_per_round"])
    res["metrics_in_launcher_us"] = 1e6 * med([t for r in with_m for t in r["metrics_frame_s"]])
    res["metrics_share_of_frame"] = res["metrics_in_launcher_us"] * 1e-3 / res["frame_f16x2_ms"]
    res["frame_delta_share_of_frame"] = (res["frame_f16x2_with_metrics_ms"] - res["frame_f16x2_ms"]) / res["frame_f16x2_ms"]
    res["kernel_share_of_frame"] = res["c_call_us"][0] * 1e-3 / res["frame_f16x2_ms"]
    res["launcher_metrics"] = with_m[-1]["metrics"]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    worst = max(res["metrics_share_of_frame"], res["frame_delta_share_of_frame"])
    if not worst <= 0.01:
        raise SystemExit(f"--metrics costs {100 * worst:.2f} % of an f16x2 frame (bound: 1 %)")


if __name__ == "__main__":
    main()

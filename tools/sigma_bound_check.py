"""How much of a frame the sigma gate (csrc/nf_mlp_gated.hip, DESIGN.md "Sigma gate") can prove dead -- on the CPU, with the oracle port,
the benchmark's weights, poses, conditioning and validation settings (bench_common): for a sample of rays of each frame the share of
points that are live (density above zero, or last on their ray) and the share the bound fails to prove, in the coarse and in the fine
pass; and that no proven point has positive density (float64 from the same h).

    python tools/sigma_bound_check.py [--frames 2 3 6] [--rays 1024]

The bound is tests/sigma_bound_ref.py's restatement in float32; the kernel sums the same terms in another order.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[2, 3, 6])
    ap.add_argument("--rays", type=int, default=1024)
    a = ap.parse_args(argv)
    from tests import sigma_bound_ref as B                                 # (the checker: it owns the oracle side of this)
    print("| frame | coarse: live / not proven | fine: live / not proven | proven with positive density |")
    print("|---|---|---|---|")
    bad = 0
    for f, (live_c, kept_c), (live_f, kept_f), wrong in B.benchmark_shares(a.frames, a.rays):
        print(f"| {f} | {live_c:.3f} / {kept_c:.3f} | {live_f:.3f} / {kept_f:.3f} | {wrong} |")
        bad += wrong
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""How long are the camera-ray candidate lists (csrc/camera_candidates.hpp) of a scene's work items?  Host only: the scene is lowered without
a device and the header's walk runs on the CPU (mi355pt_scene_debug_camera_candidates).  For each block size 1, 2, 4, 8 it draws `--blocks`
random aligned pixel blocks of the frame and prints one JSON line with the list length's mean and quantiles and the share of blocks whose
list fits the kernels' cap.

    tools/camera_list_stats.py [--scene 3] [--width 1920] [--height 1080] [--blocks 3000] [--cap 16] [--seed 0]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--blocks", type=int, default=3000)
    ap.add_argument("--cap", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    pkg = importlib.import_module("toy-cpu-pathtracing_amd")
    prod = pkg.Product()
    scene = prod.new_scene()
    cam = pkg.scenes.load_scene(scene, args.scene, args.width, args.height, build=False)
    rng = np.random.default_rng(args.seed)
    for b in (1, 2, 4, 8):
        x0 = rng.integers(0, (args.width + b - 1) // b, args.blocks) * b
        y0 = rng.integers(0, (args.height + b - 1) // b, args.blocks) * b
        rects = np.stack([x0, y0, x0 + b - 1, y0 + b - 1], axis=1)
        counts, over, _ = scene.debug_camera_candidates(cam, rects, cap=4096)
        assert not over.any()
        q = np.percentile(counts, [50, 90, 99])
        print(json.dumps({"scene": args.scene, "frame": [args.width, args.height], "block": b, "blocks": args.blocks, "mean": round(float(counts.mean()), 2),
                          "p50": int(q[0]), "p90": int(q[1]), "p99": int(q[2]), "max": int(counts.max()),
                          f"share_le_{args.cap}": round(float((counts <= args.cap).mean()), 4), "share_le_32": round(float((counts <= 32).mean()), 4)}))


if __name__ == "__main__":
    main()

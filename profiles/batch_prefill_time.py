"""Wall and device milliseconds to prefill B sequences of Qwen2-VL-2B (bench.py's synthetic weights): B in {2, 4, 8, 15} x S in {8, 24, 64} text tokens per sequence, one
mixed row (the bench's image prompt, S = 282 with its 256 tower rows handed in on the device, + 14 text prompts of 24 tokens), and the solo prefill of that image prompt.

  --mode loop    the loop `batch_select(b); prefill(...)` over the prompts: B passes over the weights (what a parent-commit library can do)
  --mode batch   ONE Model.batch_prefill call over the same prompts
  --so PATH      load this libmllm_hip.so instead of the tree's (the parent commit's build, for --mode loop)

The model is created with cache_limit = 1024 (both modes): the activation buffers hold cache_limit rows and B = 15 x S = 64 is 960.  Per cell: the caches cleared, one warm
call, then the median of 5 timed calls.  One process = one run; profiles/batch_prefill.md holds three alternating runs of each and the command lines.  Prints one JSON line.  --check (batch mode) compares every row's greedy id with the id of the same prompt prefilled alone on the same model."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loop", "batch"), required=True)
    ap.add_argument("--so", default=None)
    ap.add_argument("--batches", default="2,4,8,15")
    ap.add_argument("--lengths", default="8,24,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cache-limit", type=int, default=1024)      # 15 x 64 = 960 rows in one pass: above the config's default of 800 rows
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from mllm_amd import lib, synth
    from mllm_amd import synthfile as weights
    if args.so:
        lib.SO_PATH = os.path.abspath(args.so)
    cfg = synth.qwen2vl_2b()
    path = weights.qwen2vl_file(cfg, cache_dir=os.environ.get("MLLM_AMD_CACHE", "/tmp/mllm_amd_cache"))
    image, meta, ids_img = synth.qwen2vl_inputs(cfg, (32, 32), 24)
    m = lib.Model(cfg, path, cache_limit=args.cache_limit)
    rows, cols = m.vision_shape(meta)
    vis = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    m.vision(image, meta, vis.data_ptr(), 1)
    m.batch_begin(15)
    rng = np.random.default_rng(2024)
    text = lambda n: rng.integers(0, 151643, size=n).astype(np.int32)

    def clear(B):
        for b in range(B):
            m.batch_select(b)
            m.clear_kvcache()

    def loop(prompts, nvr):
        """-> (ids, device ms): one ordinary prefill per sequence"""
        out, dev = [], 0.0
        for b, p in enumerate(prompts):
            m.batch_select(b)
            if nvr[b]:
                tk, _, ms = m.prefill(p, None, meta, want_logits=False, visual_dev=vis.data_ptr(), n_visual_rows=int(nvr[b]))
            else:
                tk, _, ms = m.prefill(p, want_logits=False)
            out.append(tk)
            dev += ms
        return out, dev

    def batch(prompts, nvr):
        if any(nvr):
            nxt, _, ms = m.batch_prefill(prompts, visual_dev=vis, grid_thw=meta, n_visual_rows=nvr, want_logits=False)
        else:
            nxt, _, ms = m.batch_prefill(prompts, want_logits=False)
        return nxt.tolist(), ms

    def cell(prompts, nvr, call):
        B = len(prompts)
        walls, devs, got = [], [], None
        for rep in range(args.reps + 1):      # rep 0 warms
            clear(B)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got, dev = call(prompts, nvr)
            torch.cuda.synchronize()
            if rep:
                walls.append((time.perf_counter() - t0) * 1e3)
                devs.append(dev)
        res = {"wall_ms": round(statistics.median(walls), 4), "device_ms": round(statistics.median(devs), 4)}
        if args.check and call is batch:
            clear(B)
            res["rows_equal_solo"] = got == loop(prompts, nvr)[0]
        return res

    call = batch if args.mode == "batch" else loop
    out = {"mode": args.mode, "so": args.so, "reps": args.reps, "cache_limit": args.cache_limit, "cells": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        for S in [int(s) for s in args.lengths.split(",")]:
            out["cells"][f"B{B}_S{S}"] = cell([text(S) for _ in range(B)], [0] * B, call)
    out["cells"]["mixed_1x282_14x24"] = cell([ids_img] + [text(24) for _ in range(14)], [rows] + [0] * 14, call)
    # the ordinary prefill of the image prompt alone (tower rows on the device): shares no code path with the batched call, so the parent's and the tree's agree
    out["solo_prefill_S282"] = cell([ids_img], [rows], loop)
    m.batch_select(0)
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Wall milliseconds per batched decode step of Qwen2-VL-2B (bench.py's weights and prompt in every row): 8 warm steps, then 64 timed ones, for B = 2, 4, 8, 15.

  --mode decode_loop   the Python loop over Model.batch_decode(cur, want_logits=False), as bench.py --full times the batched extra (two host round trips per step)
  --mode generate      ONE Model.batch_generate call (device-resident state, one captured graph per B)
  --so PATH            load this libmllm_hip.so instead of the tree's (the parent commit's build, for decode_loop)

One process = one run; profiles/batch_generate.md holds three alternating runs of each and the command lines.  Prints one JSON line.
--check compares every row's ids with the reference's run of the bench prompt (tests/golden/qwen2vl_2b_ref.npz)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("decode_loop", "generate"), required=True)
    ap.add_argument("--so", default=None)
    ap.add_argument("--batches", default="2,4,8,15")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warm", type=int, default=8)
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
    image, meta, ids = synth.qwen2vl_inputs(cfg, (32, 32), 24)
    m = lib.Model(cfg, path)
    gold = alone = None
    if args.check:
        gold = np.load(os.path.join(ROOT, "tests", "golden", "qwen2vl_2b_ref.npz"))["tokens"].tolist()
        tk, _, _ = m.prefill(ids, image, meta, want_logits=False)      # the same model's batch-1 run (fused single-sequence step)
        alone = [tk] + m.generate(tk, args.warm + args.steps)[0].tolist()
        m.clear_kvcache()
    out = {"mode": args.mode, "so": args.so, "steps": args.steps, "warm": args.warm, "ms_per_step_wall": {}, "ms_per_step_device": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        m.batch_begin(B)
        cur = []
        for b in range(B):
            m.batch_select(b)
            m.clear_kvcache()
            tk, _, _ = m.prefill(ids, image, meta, want_logits=False)
            cur.append(tk)
        got = [[t] for t in cur]
        if args.mode == "generate":
            toks, _, _ = m.batch_generate(cur, args.warm)
            warm = toks
            cur = toks[:, -1].tolist()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks, _, dev = m.batch_generate(cur, args.steps)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            for b in range(B):
                got[b] += warm[b].tolist() + toks[b].tolist()
        else:
            for _ in range(args.warm):
                cur = m.batch_decode(cur, want_logits=False)[0].tolist()
                for b in range(B):
                    got[b].append(cur[b])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev = 0.0
            for _ in range(args.steps):
                nxt, _, ms_b = m.batch_decode(cur, want_logits=False)
                cur = nxt.tolist()
                dev += ms_b
                for b in range(B):
                    got[b].append(cur[b])
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        out["ms_per_step_wall"][B] = round(wall * 1e3 / args.steps, 4)
        out["ms_per_step_device"][B] = round(dev / args.steps, 4)
        if gold is not None:
            n = min(len(gold), len(got[0]))
            first_diff = lambda a, b: next((i for i in range(n) if a[i] != b[i]), None)
            out.setdefault("rows_equal_reference", {})[B] = all(got[b][:n] == gold[:n] for b in range(B))
            out.setdefault("rows_equal_batch1_run", {})[B] = all(got[b][:n] == alone[:n] for b in range(B))
            out.setdefault("first_id_off_the_reference", {})[B] = [first_diff(got[b], gold) for b in range(B)]
            out["batch1_run_first_id_off_the_reference"] = first_diff(alone, gold)
            out["ids_compared"] = n
    m.batch_select(0)
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Wall milliseconds per batched step of Qwen2-VL-2B (bench.py's weights and prompt in every row) for the sampled generation methods: 8 warm steps, then 64 timed ones,
for B = 2, 4, 8, 15.

  --mode sampled     ONE Model.batch_generate_sampled call (--method 1 top-k, 2 top-p; --top-k, --top-p, --temperature)
  --mode greedy      ONE Model.batch_generate call (the floor: the same step with the argmax tail)
  --mode solo_loop   what a caller had before: batch_select(b) + Model.generate_sampled for b = 0 .. B-1, one after the other; the B runs' wall time over the 64 steps

greedy and solo_loop use nothing the parent commit lacks, so the same file runs in a checkout of the parent.  One process = one run; profiles/batch_generate_sampled.md
holds three runs of each and the command lines.  Prints one JSON line.  --nucleus also prints, for --method 2, the nucleus sizes of the first step's B rows (from one
batch_decode's logits, computed on the host)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _nucleus_sizes(logits, top_p):
    out = []
    for row in logits:
        e = np.exp(row.astype(np.float64) - float(row.max()))
        p = np.sort((e / e.sum()).astype(np.float32))[::-1]
        out.append(int(min(p.size, np.searchsorted(np.cumsum(p, dtype=np.float32), np.float32(top_p)) + 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("sampled", "greedy", "solo_loop"), required=True)
    ap.add_argument("--method", type=int, default=1)
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--top-p", type=float, default=0.92)
    ap.add_argument("--temperature", type=float, default=0.7)
    ap.add_argument("--batches", default="2,4,8,15")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--nucleus", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from mllm_amd import lib, synth
    from mllm_amd import synthfile as weights
    cfg = synth.qwen2vl_2b()
    path = weights.qwen2vl_file(cfg, cache_dir=os.environ.get("MLLM_AMD_CACHE", "/tmp/mllm_amd_cache"))
    image, meta, ids = synth.qwen2vl_inputs(cfg, (32, 32), 24)
    m = lib.Model(cfg, path)
    kw = dict(top_k=args.top_k, top_p=args.top_p, temperature=args.temperature)
    out = {"mode": args.mode, "method": args.method if args.mode != "greedy" else 0, **kw, "steps": args.steps, "warm": args.warm, "ms_per_step_wall": {},
           "ms_per_step_device": {}}
    rng = np.random.default_rng(5)
    for B in [int(b) for b in args.batches.split(",")]:
        m.batch_begin(B)
        cur = []
        for b in range(B):
            m.batch_select(b)
            m.clear_kvcache()
            tk, _, _ = m.prefill(ids, image, meta, want_logits=False)
            cur.append(tk)
        uw, u = rng.random((B, args.warm)).astype(np.float32), rng.random((B, args.steps)).astype(np.float32)
        if args.nucleus and args.mode == "sampled" and args.method == 2:
            nxt, lg, _ = m.batch_decode(cur)
            cur = nxt.tolist()
            out.setdefault("nucleus_sizes_first_step", {})[B] = _nucleus_sizes(lg, args.top_p)
        if args.mode == "greedy":
            cur = m.batch_generate(cur, args.warm)[0][:, -1].tolist()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, dev = m.batch_generate(cur, args.steps)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        elif args.mode == "sampled":
            cur = m.batch_generate_sampled(cur, args.warm, args.method, uw, **kw)[0][:, -1].tolist()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, n_out, amb, dev = m.batch_generate_sampled(cur, args.steps, args.method, u, **kw)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            assert n_out.tolist() == [args.steps] * B
            out.setdefault("n_ambiguous", {})[B] = amb
        else:
            for b in range(B):
                m.batch_select(b)
                cur[b] = int(m.generate_sampled(cur[b], args.warm, args.method, uw[b], **kw)[0][-1])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev = 0.0
            for b in range(B):
                m.batch_select(b)
                toks, ms_b = m.generate_sampled(cur[b], args.steps, args.method, u[b], **kw)
                assert toks.size == args.steps
                dev += ms_b
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        out["ms_per_step_wall"][B] = round(wall * 1e3 / args.steps, 4)
        out["ms_per_step_device"][B] = round(dev / args.steps, 4)
    m.batch_select(0)
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

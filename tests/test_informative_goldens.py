"""The full-range model files (synthfile full_range=True) and the reference goldens made on them (tests/golden/qwen2vl_tiny_fr.npz, configs_tiny_fr.npz; oracle/make_golden.py
--informative), plus the 2 B runs that decode past T = 512 (qwen2vl_2b_ref.npz, qwen2vl_2b_ref_long.npz).  CPU only.

The default draw makes every model collapse onto one greedy id, so a decode step that embeds a stale token passes every golden made on it.  Here: the default files stay
byte-identical (they are the bench workload and the input of every older golden), each new golden's ids really change, and the oracle's composed graphs reproduce every stored
logit of the new tiny runs bit for bit."""
import hashlib
import os

import numpy as np
import pytest

from mllm_amd import mllmfile as mf, synth
from mllm_amd import synthfile as weights

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# sha256 (first 16 hex digits) of tensors of the default toy Qwen2-VL file, recorded before the full_range flag existed
DEFAULT_TINY_DIGESTS = {
    "model.embed_tokens.weight": "3cc7a6c775219811",                     # Q4_0
    "model.layers.0.self_attn.q_proj.weight": "b9c521497d5780e1",        # Q4_K
    "model.layers.0.self_attn.q_proj.bias": "b96bf6da7d5df85d",          # fp32
    "model.layers.1.mlp.down_proj.weight": "c22e440fac13b5bb",
    "model.norm.weight": "893a106828fbdb95",
    "visual.blocks.0.attn.qkv.weight": "4e2fa79018729ba1",
}
DEFAULT_TINY_FILE = "e9926a6b989611889d86ff6212e54092e0f83e9ecaa550683f27afcc3e846c9f"
DEFAULT_TINYLLAMA_Q4K_FILE = "a573464c64998a7ce47ccfa2672fae2812c74a95668ed40413aa09e8161ed73a"


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def test_default_files_are_unchanged_and_full_range_files_differ(tmp_path):
    cfg = synth.qwen2vl_tiny()
    path = weights.qwen2vl_file(cfg, cache_dir=str(tmp_path))
    dig = weights.tensor_digests(path)
    assert {n: dig[n] for n in DEFAULT_TINY_DIGESTS} == DEFAULT_TINY_DIGESTS
    assert _sha(path) == DEFAULT_TINY_FILE
    assert _sha(weights.causal_lm_file(synth.tinyllama_tiny(mf.Q4_K), cache_dir=str(tmp_path))) == DEFAULT_TINYLLAMA_Q4K_FILE
    fr = weights.qwen2vl_file(cfg, cache_dir=str(tmp_path), full_range=True)
    assert fr != path and weights.FULL_RANGE_TAG in os.path.basename(fr)
    dfr = weights.tensor_digests(fr)
    assert dfr.keys() == dig.keys()
    fd = mf.MllmFile(path)
    kinds = {n: fd.dtype(n) for n in dig}
    fd.close()
    for n, dt in kinds.items():
        if dt == mf.F32:           # norms and biases do not depend on the draw
            assert dfr[n] == dig[n], n
        else:
            assert dfr[n] != dig[n], n
    f = mf.MllmFile(fr)
    name = "model.layers.0.mlp.gate_proj.weight"
    assert f.dtype(name) == mf.Q4_K and f.dtype("model.embed_tokens.weight") == mf.Q4_0
    d = np.array(f.raw(name)).reshape(-1, 144)[:, :2].copy().view(np.float16).ravel()
    d0 = np.array(f.raw("model.embed_tokens.weight")).reshape(-1, 18)[:, :2].copy().view(np.float16).ravel()
    f.close()
    assert np.count_nonzero(d == 0) > 0 and np.count_nonzero(d0 == 0) > 0 and np.count_nonzero(d0 < 0) > 0


def _nondegenerate(toks):
    t = np.asarray(toks)
    return len(np.unique(t)) >= 8 and int(np.count_nonzero(t[1:] != t[:-1])) >= 12


def test_informative_goldens_are_not_degenerate():
    """Every run of >= 24 steps in the new goldens has >= 8 distinct greedy ids, and the id differs from its predecessor at >= 12 steps."""
    g = np.load(os.path.join(GOLD, "qwen2vl_tiny_fr.npz"))
    c = np.load(os.path.join(GOLD, "configs_tiny_fr.npz"))
    long2b = np.load(os.path.join(GOLD, "qwen2vl_2b_ref_long.npz"))
    runs = {"image": g["tokens"], "text": g["tokens_text"], "long": g["tokens_long"], "untied": g["tokens_untied"], "qwen15": c["qwen_tokens"],
            "tinyllama_q4k": c["tlq_tokens"], "2b_long": long2b["tokens"]}
    for k, t in runs.items():
        assert len(t) >= 24 and _nondegenerate(t), (k, t.tolist())
    assert len(g["tokens"]) == len(g["tokens_text"]) == 40 and len(g["ids_text"]) == 40
    assert len(g["ids_long"]) + len(g["tokens_long"]) - 1 > 513
    for f in ("qwen2vl_tiny_fr.npz", "configs_tiny_fr.npz", "qwen2vl_2b_ref.npz", "qwen2vl_2b_ref_long.npz"):
        assert os.path.getsize(os.path.join(GOLD, f)) <= 1_000_000, f


def test_2b_golden_covers_the_bench_run_and_keeps_its_first_65_steps():
    """qwen2vl_2b_ref.npz: the prefill's id + 256 greedy steps (the plain bench's segment), sampled logits at T = 448 / 449 / 512 / 513 (steps 166 / 167 / 230 / 231);
    its first 65 ids are those of the 65-step run it replaced, whose id changes from step 25 on."""
    g = np.load(os.path.join(GOLD, "qwen2vl_2b_ref.npz"))
    t = g["tokens"].tolist()
    assert len(t) == 257 and t[:25] == [103690] + [73842] * 24 and len(set(t[25:])) > 30
    assert hashlib.sha256(g["tokens"][:65].astype(np.int32).tobytes()).hexdigest()[:16] == "4702e0437edef109"      # the 65 ids of the run it replaced
    assert {0, 16, 32, 48, 64, 166, 167, 230, 231, 256} <= set(g["steps"].tolist())
    assert g["top_idx"].shape == (len(g["steps"]), 64) and g["strided"].shape[0] == len(g["steps"])


def _oracle_tiny(cfg):
    from oracle import models
    return models, models.Weights(weights.qwen2vl_file(cfg, full_range=True))


def _oracle_run(m, first_logits, n):
    lg = first_logits
    rows, toks = [lg], [int(lg.argmax())]
    for _ in range(n - 1):
        lg = m.decode(toks[-1])
        rows.append(lg)
        toks.append(int(lg.argmax()))
    return toks, np.stack(rows)


def test_oracle_reproduces_the_full_range_qwen2vl_goldens():
    """(a) image prompt, (b) text prompt, (d) untied head: every logit; (c) the long run at cache_limit 800: every id and the stored logits (T = 448 / 449 / 512 / 513 among them)."""
    g = np.load(os.path.join(GOLD, "qwen2vl_tiny_fr.npz"))
    cfg = synth.qwen2vl_tiny()
    models, w = _oracle_tiny(cfg)
    pix, grid, ids = synth.qwen2vl_inputs(cfg, (8, 8), 6)
    assert np.array_equal(ids, g["ids"])
    m = models.LLM(w, cfg)
    toks, rows = _oracle_run(m, m.prefill(ids, pix, grid), len(g["tokens"]))
    assert toks == g["tokens"].tolist() and np.array_equal(rows, g["logits"])
    m = models.LLM(w, cfg)
    toks, rows = _oracle_run(m, m.prefill(g["ids_text"]), len(g["tokens_text"]))
    assert toks == g["tokens_text"].tolist() and np.array_equal(rows, g["logits_text"])
    cl = synth.qwen2vl_tiny()
    cl.cache_limit = 800
    m = models.LLM(w, cl)
    toks, rows = _oracle_run(m, m.prefill(g["ids_long"]), len(g["tokens_long"]))
    assert toks == g["tokens_long"].tolist() and np.array_equal(rows[g["long_steps"]], g["logits_long"])
    cu = synth.qwen2vl_tiny()
    cu.tie_embedding = False
    models, wu = _oracle_tiny(cu)
    m = models.LLM(wu, cu)
    toks, rows = _oracle_run(m, m.prefill(ids, pix, grid), len(g["tokens_untied"]))
    assert toks == g["tokens_untied"].tolist() and np.array_equal(rows, g["logits_untied"])


@pytest.mark.parametrize("key,mk", [("qwen", synth.qwen15_tiny), ("tlq", lambda: synth.tinyllama_tiny(mf.Q4_K))], ids=["qwen", "tlq"])
def test_oracle_reproduces_the_full_range_causal_lm_goldens(key, mk):
    from oracle import models as om
    gold = np.load(os.path.join(GOLD, "configs_tiny_fr.npz"))
    cfg = mk()
    assert np.array_equal(synth.causal_lm_ids(cfg, 20), gold[key + "_ids"])
    m = om.CausalLM(om.Weights(weights.causal_lm_file(cfg, full_range=True)), cfg)
    cur = gold[key + "_ids"]
    for s, ref in enumerate(gold[key + "_logits"]):
        lg = m.forward(cur)
        assert np.array_equal(lg, ref), (s, float(np.abs(lg - ref).max()))
        assert int(np.argmax(lg)) == int(gold[key + "_tokens"][s])
        cur = [int(np.argmax(lg))]

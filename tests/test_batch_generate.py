"""Batched greedy generation resident on the device (mllm_hip_model_batch_generate): B sequences per captured step, the per-sequence state advanced by the step's last
launch, no host round trip between steps.  The contract is batch_decode's, over a whole run: ROW b EQUALS, ID FOR ID, WHAT SEQUENCE b PRODUCES STEPPING ALONE.  The
yardsticks are the full-range files and the reference's goldens on them (tests/golden/qwen2vl_tiny_fr.npz, configs_tiny_fr.npz), whose greedy ids change from step to step,
so a row that was fed a stale or a neighbour's token cannot pass.  With want = a golden's ids, first_tokens[b] = want[0] and tokens[b][s] must equal want[s + 1].  Every
comparison is array_equal / ==."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mllm_amd import mllmfile as mf, synth
from mllm_amd import synthfile as weights

pytestmark = pytest.mark.gpu
CACHE = os.environ.get("MLLM_AMD_CACHE", "/tmp/mllm_amd_cache")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _gold(name):
    return np.load(os.path.join(HERE, "golden", name))


def _alone(lib, cfg, path, prompt, steps, image=None, meta=None, cache_limit=None):
    """batch-1 run on a fresh model: prefill, then the fused single-sequence generate (one captured graph); ids [steps + 1], the prefill's first"""
    m = lib.Model(cfg, path, cache_limit=cache_limit)
    tok, _, _ = m.prefill(prompt, image, meta, want_logits=False)
    toks, _ = m.generate(tok, steps)
    m.close()
    return [tok] + toks.tolist()


def _alone_logits(lib, cfg, path, prompt, steps, image=None, meta=None):
    """batch-1 run by single decode steps: (ids [steps + 1], logits [steps + 1][vocab])"""
    m = lib.Model(cfg, path)
    tok, lg, _ = m.prefill(prompt, image, meta)
    toks, rows = [tok], [lg]
    for _ in range(steps):
        tok, lg, _ = m.decode(tok)
        toks.append(tok)
        rows.append(lg)
    m.close()
    return toks, np.stack(rows)


def _qwen2vl_case():
    """the four prompts of test_batched_rows_equal_the_reference_on_the_full_range_file: image golden, text golden, two random text prompts of 9 and 17 ids"""
    g = _gold("qwen2vl_tiny_fr.npz")
    cfg = synth.qwen2vl_tiny()
    path = weights.qwen2vl_file(cfg, CACHE, full_range=True)
    pix, grid, ids_img = synth.qwen2vl_inputs(cfg, (8, 8), 6)
    r = np.random.default_rng(78)
    prompts = [(ids_img, pix, grid), (g["ids_text"], None, None), (r.integers(0, 2000, size=9).astype(np.int32), None, None),
               (r.integers(0, 2000, size=17).astype(np.int32), None, None)]
    return g, cfg, path, prompts


def _prefill_all(m, prompts):
    m.batch_begin(len(prompts))
    first = []
    for b, p in enumerate(prompts):
        p, im, me = p if isinstance(p, tuple) else (p, None, None)
        m.batch_select(b)
        tok, _, _ = m.prefill(p, im, me, want_logits=False)
        first.append(tok)
    return first


def _plen(p):
    return len(p[0]) if isinstance(p, tuple) else len(p)


def _qwen2vl_b4_run(lib):
    """test 1's run: (generated ids [4][39], n_out, wanted ids per row [40])"""
    g, cfg, path, prompts = _qwen2vl_case()
    steps = len(g["tokens"]) - 1
    want = [g["tokens"].tolist(), g["tokens_text"].tolist()] + [_alone(lib, cfg, path, p, steps, im, me) for p, im, me in prompts[2:]]
    m = lib.Model(cfg, path)
    first = _prefill_all(m, prompts)
    assert first == [w[0] for w in want]
    toks, n_out, ms = m.batch_generate(first, steps)
    lens = []
    for b in range(4):
        m.batch_select(b)
        lens.append(m.cache_len())
    m.close()
    assert lens == [_plen(p) + steps for p in prompts]
    assert ms > 0
    return toks, n_out, want, steps


def test_qwen2vl_b4_rows_equal_the_reference_and_their_batch1_runs():
    """Qwen2-VL tiny, B = 4, 39 steps in ONE call: rows 0 and 1 equal the reference's ids for the image and the text prompt, rows 2 and 3 a batch-1 generate on a fresh
    model; every cache has grown by 39."""
    from mllm_amd import lib
    toks, n_out, want, steps = _qwen2vl_b4_run(lib)
    assert toks.shape == (4, steps) and toks.dtype == np.int32
    assert n_out.tolist() == [steps] * 4
    for b in range(4):
        assert np.array_equal(toks[b], np.asarray(want[b][1:], dtype=np.int32)), (b, toks[b].tolist(), want[b][1:])


@pytest.mark.parametrize("key,mk", [("tlq", lambda: synth.tinyllama_tiny(mf.Q4_K)), ("qwen", synth.qwen15_tiny)], ids=["tinyllama_q4k", "qwen15"])
def test_causal_lms_b2_then_b3_on_the_full_range_files(key, mk):
    """TinyLlama Q4_K (Linear head, HF rotary, GQA 4 / 2) and Qwen1.5 (tied head, q/k/v bias): the golden prompt in row 0 against the reference's 31 steps, the other
    rows against their batch-1 runs; on ONE model first B = 2 (15 steps), then B = 3 (a second graph; row 2 starts there) for the rest."""
    from mllm_amd import lib
    g = _gold("configs_tiny_fr.npz")
    cfg = mk()
    path = weights.causal_lm_file(cfg, CACHE, full_range=True)
    r = np.random.default_rng(6)
    prompts = [g[key + "_ids"]] + [r.integers(0, cfg.vocab, size=n).astype(np.int32) for n in (6, 11)]
    steps = len(g[key + "_tokens"]) - 1
    assert steps == 31
    s2 = 15
    want = [g[key + "_tokens"].tolist(), _alone(lib, cfg, path, prompts[1], steps), _alone(lib, cfg, path, prompts[2], steps - s2)]
    m = lib.Model(cfg, path)
    first = _prefill_all(m, prompts)
    assert first == [w[0] for w in want]
    t2, n2, _ = m.batch_generate(first[:2], s2)
    assert n2.tolist() == [s2, s2]
    for b in range(2):
        assert np.array_equal(t2[b], want[b][1:s2 + 1]), (b, t2[b].tolist())
    t3, n3, _ = m.batch_generate([int(t2[0][-1]), int(t2[1][-1]), first[2]], steps - s2)
    assert n3.tolist() == [steps - s2] * 3
    assert np.array_equal(t3[0], want[0][s2 + 1:]) and np.array_equal(t3[1], want[1][s2 + 1:]), (t3[0].tolist(), t3[1].tolist())
    assert np.array_equal(t3[2], want[2][1:]), t3[2].tolist()
    for b, n in enumerate((steps, steps, steps - s2)):
        m.batch_select(b)
        assert m.cache_len() == len(prompts[b]) + n
    m.close()


def test_keys_pass_the_attention_boundaries_while_the_other_row_is_short():
    """cache_limit = 640: row 0 is the 430-id prompt, whose keys pass 448 and 512 during 119 steps (the reference's ids), while row 1 starts from 9 ids (its batch-1 run)"""
    from mllm_amd import lib
    g = _gold("qwen2vl_tiny_fr.npz")
    cfg = synth.qwen2vl_tiny()
    path = weights.qwen2vl_file(cfg, CACHE, full_range=True)
    short = np.random.default_rng(79).integers(0, 2000, size=9).astype(np.int32)
    steps = len(g["tokens_long"]) - 1
    assert steps == 119 and len(g["ids_long"]) == 430
    want1 = _alone(lib, cfg, path, short, steps, cache_limit=640)
    m = lib.Qwen2VL(cfg, path, cache_limit=640)
    first = _prefill_all(m, [g["ids_long"], short])
    assert first == [int(g["tokens_long"][0]), want1[0]]
    toks, n_out, _ = m.batch_generate(first, steps)
    m.close()
    assert n_out.tolist() == [steps, steps]
    assert np.array_equal(toks[0], g["tokens_long"][1:]), toks[0].tolist()
    assert np.array_equal(toks[1], want1[1:]), toks[1].tolist()


def test_eos_stops_one_row_and_the_others_go_on():
    """eos = 1 on test 1's prompts.  The reference's image run produces id 1 as tokens[6], its text run never in 40 ids: row 0 stops after 6 steps (the eos id kept, the
    rest of the row -1, its cache at len(ids) + 6), row 1 runs all 39; rows 2 and 3: what their batch-1 runs say.  Then sequence 0 carries on alone exactly where it stopped."""
    from mllm_amd import lib
    g, cfg, path, prompts = _qwen2vl_case()
    eos = 1
    steps = len(g["tokens"]) - 1
    want = [g["tokens"].tolist(), g["tokens_text"].tolist()] + [_alone(lib, cfg, path, p, steps, im, me) for p, im, me in prompts[2:]]
    assert want[0][6] == eos and eos not in want[0][1:6] and eos not in want[1][1:]
    want_n = [(w[1:].index(eos) + 1) if eos in w[1:] else steps for w in want]
    assert want_n[0] == 6 and want_n[1] == steps
    m = lib.Model(cfg, path)
    first = _prefill_all(m, prompts)
    toks, n_out, _ = m.batch_generate(first, steps, eos=eos)
    assert n_out.tolist() == want_n
    assert min(want_n) < steps and max(want_n) == steps      # one row stopped early, one ran to the end: not vacuous
    for b in range(4):
        n = want_n[b]
        assert np.array_equal(toks[b][:n], want[b][1:n + 1]), (b, toks[b].tolist())
        assert np.all(toks[b][n:] == -1), (b, toks[b].tolist())
        m.batch_select(b)
        assert m.cache_len() == _plen(prompts[b]) + n, b
    m.batch_select(0)
    tok, lg, _ = m.decode(eos)
    assert tok == want[0][7] and np.array_equal(lg, g["logits"][7])
    m.close()


def test_a_batch_whose_rows_have_all_stopped_returns_early_and_carries_on():
    """B = 1 with eos = the id the first step produces: of 50 steps asked for one is made (n_out, the row's -1 tail, cache_len), and the sequence carries on from there"""
    from mllm_amd import lib
    g, cfg, path, prompts = _qwen2vl_case()
    m = lib.Model(cfg, path)
    first = _prefill_all(m, prompts[1:2])
    toks, n_out, _ = m.batch_generate(first, 50, eos=int(g["tokens_text"][1]))
    assert n_out.tolist() == [1] and toks[0][0] == g["tokens_text"][1] and np.all(toks[0][1:] == -1)
    m.batch_select(0)
    assert m.cache_len() == len(g["ids_text"]) + 1
    toks2, n2, _ = m.batch_generate([int(toks[0][0])], 10)      # and carries on
    assert np.array_equal(toks2[0], g["tokens_text"][2:12])
    m.close()


def test_routes_mix():
    """batch_generate(5) -> one batch_decode (ids and every logit) -> batch_generate(5) with B = 2 of the 4 -> batch_select(3) + the fused single-sequence generate: every id
    equals the uninterrupted batch-1 run of that sequence, cache_len is right after each stage"""
    from mllm_amd import lib
    g, cfg, path, prompts = _qwen2vl_case()
    total = 16
    want = [_alone_logits(lib, cfg, path, p, total, im, me) for p, im, me in prompts]
    assert want[0][0] == g["tokens"][:total + 1].tolist() and want[1][0] == g["tokens_text"][:total + 1].tolist()
    m = lib.Model(cfg, path)
    first = _prefill_all(m, prompts)

    def lens():
        out = []
        for b in range(4):
            m.batch_select(b)
            out.append(m.cache_len())
        return out
    base = [_plen(p) for p in prompts]
    t1, n1, _ = m.batch_generate(first, 5)
    for b in range(4):
        assert np.array_equal(t1[b], want[b][0][1:6]), b
    assert lens() == [x + 5 for x in base]
    nxt, lg, _ = m.batch_decode(t1[:, -1])
    for b in range(4):
        assert int(nxt[b]) == want[b][0][6] and np.array_equal(lg[b], want[b][1][6]), b
    assert lens() == [x + 6 for x in base]
    t2, n2, _ = m.batch_generate(nxt[:2], 5)
    for b in range(2):
        assert np.array_equal(t2[b], want[b][0][7:12]), b
    assert lens() == [base[0] + 11, base[1] + 11, base[2] + 6, base[3] + 6]
    m.batch_select(3)
    t3, _ = m.generate(int(nxt[3]), 10)
    assert np.array_equal(t3, want[3][0][7:17])
    assert m.cache_len() == base[3] + 16
    # sequence 0 leaves too: single decode steps from where the second batch_generate left it
    m.batch_select(0)
    tok, lg0, _ = m.decode(int(t2[0][-1]))
    assert tok == want[0][0][12] and np.array_equal(lg0, want[0][1][12])
    m.close()


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
if torch.cuda.is_available():
    torch.cuda.init()
from mllm_amd import lib
import tests.test_batch_generate as t
toks, n_out, want, steps = t._qwen2vl_b4_run(lib)
print("RESULT " + json.dumps({"toks": toks.tolist(), "n": n_out.tolist(), "want": [w[1:] for w in want]}))
"""


def test_no_graph_option_gives_the_same_ids():
    """MLLM_HIP_NO_GRAPH=1 (read once per model, so a fresh child process): the eager loop of the same step body gives test 1's ids"""
    import json
    env = dict(os.environ, MLLM_HIP_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["n"] == [39] * 4
    assert res["toks"] == res["want"]


def test_errors_leave_everything_as_it_was():
    from mllm_amd import lib
    g, cfg, path, prompts = _qwen2vl_case()
    m = lib.Model(cfg, path)
    first = _prefill_all(m, prompts)
    base = [_plen(p) for p in prompts]

    def lens():
        out = []
        for b in range(4):
            m.batch_select(b)
            out.append(m.cache_len())
        return out
    # the text golden's 40 ids + 57 steps pass the 96-entry cache; the other three would fit
    with pytest.raises(lib.MllmHipError):
        m.batch_generate(first, cfg.cache_limit - base[1] + 1)
    assert lens() == base
    with pytest.raises(lib.MllmHipError):
        m.batch_generate(first + [1], 3)          # B above batch_begin's
    with pytest.raises(lib.MllmHipError):
        m.batch_generate(first, 0)
    assert lens() == base
    toks, n_out, _ = m.batch_generate(first, 8)          # a valid call afterwards: the right ids
    assert np.array_equal(toks[0], g["tokens"][1:9]) and np.array_equal(toks[1], g["tokens_text"][1:9])
    assert lens() == [x + 8 for x in base]
    m.batch_select(2)
    m.clear_kvcache()
    with pytest.raises(lib.MllmHipError, match="has no prefill"):
        m.batch_generate(toks[:, -1], 2)          # a cleared sequence among the B
    assert lens() == [base[0] + 8, base[1] + 8, 0, base[3] + 8]
    t2, _, _ = m.batch_generate(toks[:2, -1], 4)          # the two rows in front of it still go on
    assert np.array_equal(t2[0], g["tokens"][9:13]) and np.array_equal(t2[1], g["tokens_text"][9:13])
    m.close()

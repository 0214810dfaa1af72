"""Batched prefill (mllm_hip_model_batch_prefill): the prompts of B sequences in ONE pass over the weights.  The contract is the one of tests/test_batched_decode.py:
SEQUENCE b OF A BATCHED PREFILL IS, BIT FOR BIT, WHAT batch_select(b) + prefill GIVES ALONE -- its greedy id, its whole logit row, and every K / V row it appended, shown
by decoding on.  Every assertion is array_equal / id equality against a run on a fresh Model (and against the reference's ids and logits where a golden holds the prompt);
the files are the full-range ones, whose greedy ids change from step to step, so a row fed another row's token or KV cannot pass."""
import functools
import gc
import os

import numpy as np
import pytest

from mllm_amd import mllmfile as mf, synth
from mllm_amd import synthfile as weights

pytestmark = pytest.mark.gpu
CACHE = os.environ.get("MLLM_AMD_CACHE", "/tmp/mllm_amd_cache")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _heads8():
    """heads = 8 at hidden 512 (D = 64, GQA 8 / 2): a head count that is a multiple of 8 takes the attention kernel's XCD head remap"""
    return synth.CausalLMConfig(family="tinyllama", hidden=512, inter=512, layers=2, heads=8, kv_heads=2, vocab=1024, rope_theta=10000.0, cache_limit=96,
                                tie_embedding=False, target=mf.Q4_K)


CONFIGS = {"qwen2vl": synth.qwen2vl_tiny, "tinyllama": lambda: synth.tinyllama_tiny(mf.Q4_K), "qwen15": synth.qwen15_tiny, "heads8": _heads8}


@functools.lru_cache(maxsize=None)
def _setup(name):
    cfg = CONFIGS[name]()
    path = weights.qwen2vl_file(cfg, CACHE, full_range=True) if name == "qwen2vl" else weights.causal_lm_file(cfg, CACHE, full_range=True)
    return cfg, path


def _prompt(name, n, seed):
    cfg, _ = _setup(name)
    return np.random.default_rng(seed).integers(0, min(cfg.vocab, 2000), size=n).astype(np.int32)


_SOLO = {}      # the solo runs the tests share; released when the module is done (the logit rows are not kept for the rest of the session)


@pytest.fixture(scope="module", autouse=True)
def _release_shared_runs():
    yield
    _SOLO.clear()
    gc.collect()


def _solo(name, turns, steps, cache_limit=None):
    """The reference every test compares with, computed once per (model, prompts) and shared: see _solo_run"""
    key = (name, turns, steps, cache_limit)
    if key not in _SOLO:
        _SOLO[key] = _solo_run(name, turns, steps, cache_limit)
    return _SOLO[key]


def _solo_run(name, turns, steps, cache_limit):
    """A fresh Model, one ordinary prefill per turn ((n, seed) -> _prompt; "img" / "text" / "tlq" / "qwen" -> the goldens' prompts), then `steps` single decode steps (the
    fused kernels).  -> ([id per turn], [logit row per turn], [decode ids], [decode rows])"""
    from mllm_amd import lib
    cfg, path = _setup(name)
    m = lib.Model(cfg, path, cache_limit=cache_limit)
    toks, rows = [], []
    for t in turns:
        if t == "img":
            pix, grid, ids = synth.qwen2vl_inputs(cfg, (8, 8), 6)
            tok, lg, _ = m.prefill(ids, pix, grid)
        else:
            tok, lg, _ = m.prefill(_ids(name, t))
        toks.append(tok)
        rows.append(lg)
    dt, dr = [], []
    for _ in range(steps):
        tok, lg, _ = m.decode(tok)
        dt.append(tok)
        dr.append(lg)
    m.close()
    return toks, rows, dt, dr


def _ids(name, t):
    if t == "text":
        return np.load(os.path.join(GOLD, "qwen2vl_tiny_fr.npz"))["ids_text"]
    if t in ("tlq", "qwen"):
        return np.load(os.path.join(GOLD, "configs_tiny_fr.npz"))[t + "_ids"]
    return _prompt(name, *t)


def _check_prefill(nxt, lg, want, turn=0):
    for b, w in enumerate(want):
        assert int(nxt[b]) == w[0][turn], (b, int(nxt[b]), w[0][turn])
        assert np.array_equal(lg[b], w[1][turn]), (b, float(np.abs(lg[b] - w[1][turn]).max()))


def _check_decode(m, cur, want, steps):
    """`steps` batch_decode steps: every id and logit row equals the solo runs' -- which proves every K row and V column the prefill appended"""
    for s in range(steps):
        nxt, lg, _ = m.batch_decode(cur)
        for b, w in enumerate(want):
            assert int(nxt[b]) == w[2][s], (s, b)
            assert np.array_equal(lg[b], w[3][s]), (s, b, float(np.abs(lg[b] - w[3][s]).max()))
        cur = nxt.tolist()
    return cur


def test_row_block_and_tiling_edges_d128():
    """qwen2vl_tiny (D = 128, GQA 2 / 1, M-RoPE, tied head), B = 9: both Br = 1 lengths (1, 3), Sq = 4 (the first 32-row form), Sk % 4 != 0, 31 / 32 / 33 (one to two row
    blocks; workgroups of the shorter sequences leave early), the fp16 left = Sk % Tc rule at several Sk."""
    from mllm_amd import lib
    cfg, path = _setup("qwen2vl")
    lens = (1, 3, 4, 5, 17, 31, 32, 33, 40)
    turns = [((n, 100 + n),) for n in lens]
    want = [_solo("qwen2vl", t, 6, 256) for t in turns]
    m = lib.Model(cfg, path, cache_limit=256)
    m.batch_begin(len(lens))
    nxt, lg, _ = m.batch_prefill([_ids("qwen2vl", t[0]) for t in turns])
    _check_prefill(nxt, lg, want)
    _check_decode(m, nxt.tolist(), want, 6)
    m.close()


def test_gemv_rows_15_and_first_gemm_rows_16():
    """R = 15 rows: every Linear takes the GEMV form; R = 16 on fresh sequences: the first row count of the packed GEMM"""
    from mllm_amd import lib
    cfg, path = _setup("qwen2vl")
    m = lib.Model(cfg, path)
    m.batch_begin(3)
    for lens in ((5, 4, 6), (5, 4, 7)):
        turns = [((n, 200 + 10 * i + n),) for i, n in enumerate(lens)]
        want = [_solo("qwen2vl", t, 2) for t in turns]
        for b in range(3):
            m.batch_select(b)
            m.clear_kvcache()
        nxt, lg, _ = m.batch_prefill([_ids("qwen2vl", t[0]) for t in turns])
        _check_prefill(nxt, lg, want)
        _check_decode(m, nxt.tolist(), want, 2)
    m.close()


def test_gemv_rows_with_the_linear_head():
    """TinyLlama (Linear Q4_K head), B = 4 with prompts of 3 and 5 ids: R = 14 rows, so every Linear of the pass takes the GEMV form and the Linear head runs over the four
    gathered rows; three batch_decode steps on (B = 4: the step's packed GEMM)."""
    from mllm_amd import lib
    cfg, path = _setup("tinyllama")
    turns = [((n, 300 + i),) for i, n in enumerate((3, 5, 3, 3))]
    want = [_solo("tinyllama", t, 3) for t in turns]
    m = lib.Model(cfg, path)
    m.batch_begin(4)
    nxt, lg, _ = m.batch_prefill([_ids("tinyllama", t[0]) for t in turns])
    _check_prefill(nxt, lg, want)
    _check_decode(m, nxt.tolist(), want, 3)
    m.close()


CASE3 = {"tinyllama": ("tlq", (6, 31), (11, 32)), "qwen15": ("qwen", (6, 33), (11, 34)), "heads8": ((40, 35), (6, 36), (33, 37))}
TURN2 = ((3, 41), (9, 42), (33, 43))


@pytest.mark.parametrize("name", ["tinyllama", "qwen15", "heads8"])
def test_d64_linear_and_tied_heads_hf_rotary_then_batch_generate(name):
    """D = 64 with HF rotary: TinyLlama (GQA 4 / 2, Linear Q4_K head), Qwen1.5 (4 / 4 heads, q/k/v bias, tied head) -- the golden prompt of configs_tiny_fr.npz is row 0 and
    equals the reference -- and 8 / 2 heads at hidden 512 (the XCD head remap, two row blocks); B = 3, then batch_generate for 5 steps against the solo runs' ids."""
    from mllm_amd import lib
    cfg, path = _setup(name)
    turns = [(t,) for t in CASE3[name]]
    want = [_solo(name, t, 5) for t in turns]
    m = lib.Model(cfg, path)
    m.batch_begin(3)
    nxt, lg, _ = m.batch_prefill([_ids(name, t[0]) for t in turns])
    _check_prefill(nxt, lg, want)
    if name != "heads8":
        g = np.load(os.path.join(GOLD, "configs_tiny_fr.npz"))
        key = CASE3[name][0]
        assert int(nxt[0]) == int(g[key + "_tokens"][0]) and np.array_equal(lg[0], g[key + "_logits"][0])
    toks, n, _ = m.batch_generate(nxt, 5)
    for b, w in enumerate(want):
        assert n[b] == 5 and toks[b].tolist() == w[2], (b, toks[b].tolist(), w[2])
    if name != "heads8":
        assert toks[0].tolist() == g[key + "_tokens"][1:6].tolist()
    m.close()


def test_second_turn_appends_to_caches_of_different_lengths():
    """T0_b > 0 and Sk != Sq: after a first batched prefill of (20, 6, 11) tokens a second one appends (3, 9, 33) -- a Br = 1 sequence over 20 cached keys, and a two-row-block
    one -- and equals solo prefill calls appending the same tokens to solo-built caches; three decode steps on."""
    from mllm_amd import lib
    cfg, path = _setup("tinyllama")
    turns = [(a, b) for a, b in zip(CASE3["tinyllama"], TURN2)]
    want = [_solo("tinyllama", t, 3) for t in turns]
    m = lib.Model(cfg, path)
    m.batch_begin(3)
    for k in range(2):
        nxt, lg, _ = m.batch_prefill([_ids("tinyllama", t[k]) for t in turns])
        _check_prefill(nxt, lg, want, k)
    for b, t in enumerate(turns):
        m.batch_select(b)
        assert m.cache_len() == sum(len(_ids("tinyllama", x)) for x in t)
    _check_decode(m, nxt.tolist(), want, 3)
    m.close()


def test_image_and_text_prompts_mixed():
    """B = 4 on qwen2vl_tiny: the golden's image prompt (its tower output computed by Model.vision into a device tensor), the golden's text prompt, two random text prompts.
    Rows 0 and 1 equal the reference (tests/golden/qwen2vl_tiny_fr.npz), the others their solo runs; four batch_decode steps."""
    import torch
    from mllm_amd import lib
    g = np.load(os.path.join(GOLD, "qwen2vl_tiny_fr.npz"))
    cfg, path = _setup("qwen2vl")
    pix, grid, ids_img = synth.qwen2vl_inputs(cfg, (8, 8), 6)
    turns = [("img",), ("text",), ((9, 51),), ((17, 52),)]
    want = [_solo("qwen2vl", t, 4) for t in turns]
    for w, tk, lk in ((want[0], "tokens", "logits"), (want[1], "tokens_text", "logits_text")):      # the solo runs are the reference's
        assert [w[0][0]] + w[2] == g[tk][:5].tolist() and np.array_equal(np.stack([w[1][0]] + w[3]), g[lk][:5])
    m = lib.Model(cfg, path)
    rows, cols = m.vision_shape(grid)
    vis = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    m.vision(pix, grid, vis.data_ptr(), 1)
    m.batch_begin(4)
    prompts = [ids_img] + [_ids("qwen2vl", t[0]) for t in turns[1:]]
    nxt, lg, _ = m.batch_prefill(prompts, visual_dev=vis, grid_thw=grid, n_visual_rows=[rows, 0, 0, 0])
    _check_prefill(nxt, lg, want)
    assert int(nxt[0]) == int(g["tokens"][0]) and np.array_equal(lg[0], g["logits"][0])
    assert int(nxt[1]) == int(g["tokens_text"][0]) and np.array_equal(lg[1], g["logits_text"][0])
    _check_decode(m, nxt.tolist(), want, 4)
    m.close()


def test_hand_over_to_the_single_sequence_step_and_untouched_sequences():
    """After a batched prefill of sequences 0 .. 2 (sequence 1 selected while it ran): the selected sequence decodes on with the fused single-sequence step without being
    selected again (needs_arm), batch_select(2) + decode x 3 equals the solo run, cache_len of every sequence is T0 + S, and sequence 3 -- outside the call, prefilled
    alone before it -- is untouched: its later decode equals its solo run."""
    from mllm_amd import lib
    cfg, path = _setup("tinyllama")
    turns = [(t,) for t in CASE3["tinyllama"]] + [((13, 61),)]
    want = [_solo("tinyllama", t, 5) for t in turns]          # (five steps: the runs test_d64_... already made; three are used)
    m = lib.Model(cfg, path)
    m.batch_begin(4)
    m.batch_select(3)
    tok3, lg3, _ = m.prefill(_ids("tinyllama", turns[3][0]))
    assert tok3 == want[3][0][0] and np.array_equal(lg3, want[3][1][0])
    m.batch_select(1)
    nxt, lg, _ = m.batch_prefill([_ids("tinyllama", t[0]) for t in turns[:3]])
    _check_prefill(nxt, lg, want[:3])
    assert m.cache_len() == 6
    for b in (1, 2, 3, 0):
        if b != 1:
            m.batch_select(b)
        assert m.cache_len() == len(_ids("tinyllama", turns[b][0]))
        tok = int(nxt[b]) if b < 3 else tok3
        for s in range(3):
            tok, row, _ = m.decode(tok)
            assert tok == want[b][2][s] and np.array_equal(row, want[b][3][s]), (b, s)
    m.close()


def test_refusals_leave_everything_as_it_was():
    """Every refused call raises and leaves cache_len of every sequence as it was; a correct call afterwards gives the solo bits."""
    from mllm_amd import lib
    import torch
    cfg, path = _setup("tinyllama")
    first = [(10, 71), (10, 72), (10, 73)]
    second = [(4, 74), (20, 75), (2, 76)]
    want = [_solo("tinyllama", t, 0) for t in zip(first, second)]
    P = lambda n, s=0: _prompt("tinyllama", n, 80 + s)
    m = lib.Model(cfg, path)          # cache_limit 96
    m.batch_begin(3)
    nxt, lg, _ = m.batch_prefill([_ids("tinyllama", t) for t in first])
    _check_prefill(nxt, lg, want, 0)
    dev = torch.zeros((16, cfg.hidden), dtype=torch.float32, device="cuda")
    bad = [
        dict(prompts=[P(40, 1), P(40, 2), P(20, 3)]),                       # 100 rows > cache_limit = 96 (every T0 + S fits)
        dict(prompts=[P(5, 1), P(87, 2), P(4, 3)]),                         # 96 rows, but 10 + 87 > 96
        dict(prompts=[P(5, 1), P(5, 2), P(5, 3), P(5, 4)]),                 # B above batch_begin's
        dict(prompts=[P(5, 1), np.zeros(0, np.int32), P(5, 3)]),            # an empty prompt
        dict(prompts=[P(16, 1), P(5, 2), P(5, 3)], visual_dev=dev, grid_thw=[1, 8, 8], n_visual_rows=[16, 0, 0]),      # visual rows on a model without a tower
    ]
    for kw in bad:
        with pytest.raises(lib.MllmHipError):
            m.batch_prefill(**kw)
        for b in range(3):
            m.batch_select(b)
            assert m.cache_len() == 10, (kw, b)
    nxt, lg, _ = m.batch_prefill([_ids("tinyllama", t) for t in second])
    _check_prefill(nxt, lg, want, 1)
    m.close()
    # a wrong image-token count (Qwen2-VL): one image token short of the tower's rows; and image tokens without any visual rows
    cfg, path = _setup("qwen2vl")
    pix, grid, ids_img = synth.qwen2vl_inputs(cfg, (8, 8), 6)
    text = _ids("qwen2vl", (9, 51))
    want = [_solo("qwen2vl", ("img",), 4), _solo("qwen2vl", ((9, 51),), 4)]
    m = lib.Model(cfg, path)
    rows, cols = m.vision_shape(grid)
    vis = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    m.vision(pix, grid, vis.data_ptr(), 1)
    m.batch_begin(2)
    short = np.delete(ids_img, 1)
    for kw in (dict(prompts=[short, text], visual_dev=vis, grid_thw=grid, n_visual_rows=[rows, 0]), dict(prompts=[ids_img, text]),
               dict(prompts=[ids_img, text], visual_dev=vis, grid_thw=grid, n_visual_rows=[rows - 1, 0])):
        with pytest.raises(lib.MllmHipError):
            m.batch_prefill(**kw)
        for b in range(2):
            m.batch_select(b)
            assert m.cache_len() == 0
    nxt, lg, _ = m.batch_prefill([ids_img, text], visual_dev=vis, grid_thw=grid, n_visual_rows=[rows, 0])
    _check_prefill(nxt, lg, want)
    m.close()

"""Batched sampled generation (mllm_hip_sample_rows, mllm_hip_model_batch_generate_sampled): top-k / top-p candidates, the candidate softmax and the draw on the device,
per row, inside batch_generate's captured step.  The yardsticks: the reference's own candidates and probabilities (tests/golden/sampling.npz), the host functions the
single-sequence path runs (mllm_hip_topk_probs_host, mllm_hip_sample_index_host), the oracle's restatement, and -- for the engine -- ROW b EQUALS, ID FOR ID, WHAT
generate_sampled PRODUCES FOR SEQUENCE b ALONE on the same uniform numbers.  Every comparison is array_equal / ==.

The one place where equality is conditional is the double exp of the candidate softmax: the device library's and libm's are both within 1 ulp, so they round to the same
float unless the value lies within 2 double ulps of a float rounding tie; the kernels count such values (n_ambiguous), and the tests ask for 0."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from mllm_amd import mllmfile as mf, synth
from mllm_amd import synthfile as weights

CACHE = os.environ.get("MLLM_AMD_CACHE", "/tmp/mllm_amd_cache")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
gpu = pytest.mark.gpu


def _gold(name):
    return np.load(os.path.join(HERE, "golden", name))


G = _gold("sampling.npz")
K, P, T = int(G["k"]), float(G["p"]), float(G["temp"])


def _host_probs(val, temperature):
    from mllm_amd import lib
    v = np.ascontiguousarray(val, dtype=np.float32)
    p = np.empty_like(v)
    lib.check(lib.load().mllm_hip_topk_probs_host(lib.vp(v), C.c_int(v.size), C.c_float(temperature), lib.vp(p)), "topk_probs_host")
    return p


def _host_draw(prob, u):
    from mllm_amd import lib
    p = np.ascontiguousarray(prob, dtype=np.float32)
    return int(lib.load().mllm_hip_sample_index_host(lib.vp(p), C.c_int(p.size), C.c_float(u)))


# ---- 1. the op against the reference's goldens ---------------------------------------------------------------------------------------------------------------------------
def _check_topk_golden(ci, cp, cn, rows=range(4)):
    for j, i in enumerate(rows):
        assert cn[j] == K
        assert np.array_equal(ci[j, :K], G[f"topk_l{i}_idx"].astype(np.int32)), i
        assert np.array_equal(cp[j, :K], G[f"topk_l{i}_prob"]), i


def _check_topp_golden(ci, cp, cn, rows=range(4)):
    for j, i in enumerate(rows):
        want = G[f"topp_{i}_idx"].astype(np.int32)
        assert cn[j] == want.size, (i, cn[j])
        assert np.array_equal(ci[j, :want.size], want), i
        if want.size > 1:
            assert np.array_equal(cp[j, :want.size], G[f"topp_{i}_prob"]), i


@gpu
def test_op_reproduces_the_references_candidates_and_probabilities():
    """all four golden rows in one call per method, then with a row pitch above n, then row by row: the reference's candidate ids and pre-draw probabilities each time
    (nuclei of 4, 578, 1330 and 2 candidates: the sequential walks run well past one wave)"""
    from mllm_amd import ops
    assert [G[f"topp_{i}_idx"].size for i in range(4)] == [4, 578, 1330, 2]
    u = np.zeros(4, dtype=np.float32)
    n = G["logits"].shape[1]
    ids, ci, cp, cn, amb = ops.sample_rows(G["logits"], 1, u, top_k=K, temperature=T)
    _check_topk_golden(ci, cp, cn)
    assert amb == 0 and np.array_equal(ids, ci[:, 0])          # u = 0 draws the first candidate
    ids, ci, cp, cn, amb = ops.sample_rows(G["probs"], 2, u, top_p=P, temperature=T)
    _check_topp_golden(ci, cp, cn)
    assert amb == 0 and np.array_equal(ids, ci[:, 0])
    pad = np.full((4, n + 12), 7.0, dtype=np.float32)          # the columns behind n would win every selection if they were read
    for src, method, chk in ((G["logits"], 1, _check_topk_golden), (G["probs"], 2, _check_topp_golden)):
        pad[:, :n] = src
        _, ci, cp, cn, amb = ops.sample_rows(pad, method, u, top_k=K, top_p=P, temperature=T, n=n)
        chk(ci, cp, cn)
        assert amb == 0
        for i in range(4):
            _, ci, cp, cn, amb = ops.sample_rows(src[i:i + 1], method, u[:1], top_k=K, top_p=P, temperature=T)
            chk(ci, cp, cn, rows=[i])
            assert amb == 0


# ---- 2. the draw -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _draw_points(prob):
    """0, the largest float below 1, every boundary of the CDF as mllm_hip_sample_index_host accumulates it (rounded to float) and its float neighbour on either side"""
    s = 0.0
    for p in prob:
        s += float(p)
    us, acc = [0.0, 0.99999994], 0.0
    for p in prob:
        acc += float(p) / s
        b = np.float32(acc)
        us += [b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(2))]
    u = np.asarray(us, dtype=np.float32)
    return u[(u >= 0) & (u < 1)]


@gpu
@pytest.mark.parametrize("method", [1, 2], ids=["topk", "topp"])
def test_draw_equals_the_host_function_at_every_cdf_boundary(method):
    from mllm_amd import ops
    for i in range(4):
        src = G["logits"][i] if method == 1 else G["probs"][i]
        idx = (G[f"topk_l{i}_idx"] if method == 1 else G[f"topp_{i}_idx"]).astype(np.int32)
        prob = G[f"topk_l{i}_prob"] if method == 1 else G[f"topp_{i}_prob"]
        u = _draw_points(prob)
        assert u.size >= 3 * idx.size
        want = np.array([idx[_host_draw(prob, float(x))] for x in u], dtype=np.int32)
        assert len(set(want.tolist())) == idx.size          # every candidate is drawn by some u
        got = []
        for lo in range(0, u.size, 1024):          # the same row under each u, 1024 rows per call
            part = u[lo:lo + 1024]
            ids, _, _, _, amb = ops.sample_rows(np.broadcast_to(src, (part.size, src.size)), method, part, top_k=K, top_p=P, temperature=T)
            assert amb == 0
            got.append(ids)
        assert np.array_equal(np.concatenate(got), want), (method, i)


# ---- 3. selection edges ----------------------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_selection_edges():
    """k in {0, 1}: the first-maximum argmax with ties; k = 64; n = k = 7; n = 16390 and 151936 (two stages: 128 slices, then the fold) with ties at the top that lie in
    different slices and -inf entries; candidates and probabilities against the oracle's restatement, per row"""
    from mllm_amd import ops
    from oracle import oracle as orc
    r = np.random.default_rng(11)

    def check(x, k, temperature=0.7):
        ids, ci, cp, cn, amb = ops.sample_rows(x, 1, np.zeros(x.shape[0], dtype=np.float32), top_k=k, temperature=temperature)
        assert amb == 0
        for b in range(x.shape[0]):
            want_idx, _, want_p = orc.topk_sampling_probs(x[b], k, temperature)
            assert cn[b] == k and np.array_equal(ci[b, :k], want_idx) and np.array_equal(cp[b, :k], want_p), (x.shape, k, b)
            assert ids[b] == want_idx[0]

    x = r.standard_normal((3, 2048)).astype(np.float32)
    x[0, [1500, 17, 900]] = 9.0          # ties: the first maximum is index 17
    x[1, 2047] = 9.0
    for k in (0, 1):
        ids, ci, cp, cn, amb = ops.sample_rows(x, 1, np.full(3, 0.9, dtype=np.float32), top_k=k)
        assert ids.tolist() == [17, 2047, int(np.argmax(x[2]))] and cn.tolist() == [1, 1, 1] and amb == 0
    check(x, 64)
    check(r.standard_normal((2, 7)).astype(np.float32), 7)
    for n in (16390, 151936):
        x = (r.standard_normal((2, n)) * 3).astype(np.float32)
        per = (n + 127) // 128
        x[0, [5 * per + 3, 2, 127 * per + 1, 64 * per]] = 40.0          # four equal maxima in four slices
        x[0, [per - 1, per]] = 39.0                                      # and a tie across a slice edge
        x[1, n - 1] = 41.0
        x[1, 0] = 41.0
        x[:, 100:400] = -np.inf
        x[1, n // 2:n // 2 + 3000] = -np.inf
        check(x, 5)
        check(x, 64, 1.5)


# ---- 3b. top-p from logits: vocabulary softmax, whole-row sort and nucleus walk at the product's row lengths, several rows ------------------------------------------------
def _topp_from_logits_want(row, top_p, temperature, u):
    """the single-row ops the single-sequence path is built from, and the host functions: (candidate ids, probabilities, drawn id)"""
    from mllm_amd import ops
    p = ops.softmax(np.ascontiguousarray(row)).cpu().numpy().reshape(-1)      # one row: mllm_hip_softmax's own launch
    order = np.argsort(-p, kind="stable").astype(np.int32)                    # descending, equal values by ascending index: mllm_hip_sort_desc's order
    val = p[order]
    run = np.cumsum(val, dtype=np.float32)                                    # sequential float adds: `while (p < top_p) p += val[n++]`
    cnt = min(val.size, int(np.searchsorted(run, np.float32(top_p), side="left")) + 1)
    prob = _host_probs(val[:cnt], temperature) if cnt > 1 else np.ones(1, dtype=np.float32)
    return order[:cnt], prob, int(order[_host_draw(prob, u)])


@gpu
@pytest.mark.parametrize("n,rows,extra,top_ps", [(2048, 3, 0, (0.92,)), (2048, 3, 12, (0.92, 2.0)), (16390, 3, 0, (0.92, 0.9999)), (16390, 2, 10, (0.9999, 2.0)),
                                                 (151936, 3, 0, (0.92, 2.0)), (151936, 2, 24, (0.99,))],
                         ids=["short", "short_pitch", "long", "long_pitch", "vocab", "vocab_pitch"])
def test_topp_from_logits_rows_equal_the_single_row_ops(n, rows, extra, top_ps):
    """method 2 with the leading vocabulary softmax, the engine's form, on two or three rows per call: one wave per row below 16384 values (row by row when the pitch is
    not n), the chip per row from 16384 on (n = 16390: the smallest such rows; n = 151936: the product's vocabulary), with a row pitch above n whose padding would own
    the softmax if it were read.  Per row: the candidates are the single-row softmax's values in the stable descending order cut where the float running sum reaches
    top_p -- 0.92, 0.99 / 0.9999 (nuclei of many 512-value passes) and 2.0 (the whole row, the workspace's worst case, with the zero-probability ties at its end) -- and
    probabilities and draw are the host functions'.  (No candidate of these rows lies near a float rounding tie: about 2^-26 each; the test asks for 0 flags.)"""
    from mllm_amd import ops
    r = np.random.default_rng(31 + n)
    x = np.full((rows, n + extra), 60.0, dtype=np.float32)
    x[:, :n] = (r.standard_normal((rows, n)) * 3).astype(np.float32)
    x[0, [5, n - 7]] = x[0, 1000]                      # equal probabilities far apart: ascending index order
    x[1, 300:340] = -np.inf                            # probability 0: ties at the very end of the sorted row
    x[rows - 1, n - 1] = 14.0                          # the last column holds the maximum of the last row
    u = np.asarray([0.0, 0.61, 0.97][:rows], dtype=np.float32)
    for top_p in top_ps:
        ids, ci, cp, cn, amb = ops.sample_rows(x, 2, u, top_p=top_p, temperature=T, softmax_first=True, n=n)
        assert amb == 0
        sizes = []
        for b in range(rows):
            want_idx, want_p, want_id = _topp_from_logits_want(x[b, :n], top_p, T, float(u[b]))
            k = want_idx.size
            sizes.append(k)
            assert cn[b] == k, (top_p, b, cn[b], k)
            assert np.array_equal(ci[b, :k], want_idx), (top_p, b)
            if k > 1:
                assert np.array_equal(cp[b, :k], want_p), (top_p, b)
            assert ids[b] == want_id, (top_p, b)
        if top_p == 2.0:
            assert sizes == [n] * rows
        elif top_p >= 0.99 and n >= 16390:
            assert min(sizes) > 4 * 512


# ---- 4. the candidate softmax against the host function --------------------------------------------------------------------------------------------------------------------
SOFTMAX_SEED, N_SETS = 0, 2000
TEMPS = (0.3, 0.7, 1.5)


@functools.lru_cache(maxsize=None)
def _candidate_sets():
    """2,000 candidate sets, k from 2 to 64, values standard_normal * 4 in descending order (what a selection hands over); set i takes TEMPS[i % 3]"""
    r = np.random.default_rng(SOFTMAX_SEED)
    sets = []
    for i in range(N_SETS):
        k = int(r.integers(2, 65))
        v = (r.standard_normal(k) * 4).astype(np.float32)
        sets.append((v[np.argsort(-v.astype(np.float64), kind="stable")], TEMPS[i % 3]))
    return sets


def _ulps_from_float_tie(d):
    """distance, in ulps of the double d, from the nearest float rounding tie (ref_arith.h f32_rounding_ambiguous measures the same); None where no tie is near"""
    bits = np.float64(d).view(np.uint64).item()
    be = (bits >> 52) & 0x7ff
    if be == 0 or be == 0x7ff:
        return None
    e = be - 1023
    drop = 29 if e >= -126 else 29 + (-126 - e)
    if drop > 54:
        return None
    sig = (bits & ((1 << 52) - 1)) | (1 << 52)
    return abs((sig & ((1 << drop) - 1)) - (1 << (drop - 1)))


def test_the_hosts_exp_puts_no_candidate_near_a_float_tie():
    """CPU: for the seed above, libm's exp (math.exp) of every candidate of every set lies MORE than 4 double ulps from a float rounding tie.  The device's exp is within
    2 ulps of libm's (each within 1 of the true value), so it lies more than 2 ulps from the tie: the device flags nothing, and the cap of 1 ambiguous set in the GPU test
    below holds for the reference side alone."""
    near = 0
    for v, temperature in _candidate_sets():
        t = float(np.float32(temperature))
        for x in v:
            d = _ulps_from_float_tie(math.exp((float(x) - float(v[0])) / t))
            near += d is not None and d <= 4
    assert near == 0


@gpu
def test_candidate_softmax_equals_the_host_function():
    from mllm_amd import ops
    sets = _candidate_sets()
    groups = {}
    for i, (v, temperature) in enumerate(sets):
        groups.setdefault((v.size, temperature), []).append(i)
    flagged = compared = 0
    for (k, temperature), members in groups.items():
        x = np.stack([sets[i][0] for i in members])
        u = np.zeros(len(members), dtype=np.float32)
        _, ci, cp, cn, amb = ops.sample_rows(x, 1, u, top_k=k, temperature=temperature)
        assert np.array_equal(ci, np.broadcast_to(np.arange(k, dtype=np.int32), ci.shape)) and np.all(cn == k)
        for j, i in enumerate(members):
            if amb:          # some set of this call was flagged: find which, one row per call
                _, _, cp1, _, amb1 = ops.sample_rows(x[j:j + 1], 1, u[:1], top_k=k, temperature=temperature)
                if amb1:
                    flagged += 1
                    continue
                assert np.array_equal(cp1[0], cp[j])
            assert np.array_equal(cp[j], _host_probs(sets[i][0], temperature)), i
            compared += 1
    assert flagged <= 1 and flagged + compared == N_SETS


# ---- 5 .. 9: the engine ------------------------------------------------------------------------------------------------------------------------------------------------------
U_SEED, TEMP_HOT = 2025, 1.5


def _qwen2vl_case():
    """the four prompts of tests/test_batch_generate.py: image golden, text golden, two random text prompts of 9 and 17 ids"""
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


def _lens(m, B):
    out = []
    for b in range(B):
        m.batch_select(b)
        out.append(m.cache_len())
    return out


def _steps_and_u():
    g = _gold("qwen2vl_tiny_fr.npz")
    steps = len(g["tokens"]) - 1
    return steps, np.random.default_rng(U_SEED).random((4, steps)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _greedy_want():
    """ids [steps + 1] per row: the reference's for rows 0 and 1, a batch-1 greedy run on a fresh model for rows 2 and 3"""
    from mllm_amd import lib
    g, cfg, path, prompts = _qwen2vl_case()
    steps = len(g["tokens"]) - 1
    want = [g["tokens"].tolist(), g["tokens_text"].tolist()]
    for p, im, me in prompts[2:]:
        m = lib.Model(cfg, path)
        tok, _, _ = m.prefill(p, im, me, want_logits=False)
        toks, _ = m.generate(tok, steps)
        m.close()
        want.append([tok] + toks.tolist())
    return want


@functools.lru_cache(maxsize=None)
def _solo(method, eos=-1):
    """the yardstick: generate_sampled of every row alone on a fresh model, on row b's uniform numbers at temperature 1.5: (first ids, [ids of row b])"""
    from mllm_amd import lib
    _, cfg, path, prompts = _qwen2vl_case()
    steps, u = _steps_and_u()
    first, rows = [], []
    for b, (p, im, me) in enumerate(prompts):
        m = lib.Model(cfg, path)
        tok, _, _ = m.prefill(p, im, me, want_logits=False)
        toks, _ = m.generate_sampled(tok, steps, method, u[b], temperature=TEMP_HOT, eos=eos)
        m.close()
        first.append(tok)
        rows.append(toks.tolist())
    return first, rows


def _b4_sampled_run(lib, method):
    """B = 4 on the random uniform numbers at temperature 1.5 in one call: (ids [4][steps], n_out, n_ambiguous, cache lengths afterwards)"""
    _, cfg, path, prompts = _qwen2vl_case()
    steps, u = _steps_and_u()
    m = lib.Model(cfg, path)
    first = _prefill_all(m, prompts)
    toks, n_out, amb, ms = m.batch_generate_sampled(first, steps, method, u, temperature=TEMP_HOT)
    lens = _lens(m, 4)
    m.close()
    assert ms > 0
    return toks, n_out, amb, lens


@gpu
@pytest.mark.parametrize("method", [0, 1, 2], ids=["greedy", "topk", "topp"])
def test_with_u_zero_every_method_writes_the_greedy_ids(method):
    """u01 = 0 draws the first candidate = the largest score: rows 0 and 1 equal the reference's ids on the full-range file, rows 2 and 3 their batch-1 greedy runs"""
    from mllm_amd import lib
    _, cfg, path, prompts = _qwen2vl_case()
    want = _greedy_want()
    steps = len(want[0]) - 1
    m = lib.Model(cfg, path)
    first = _prefill_all(m, prompts)
    assert first == [w[0] for w in want]
    toks, n_out, amb, _ = m.batch_generate_sampled(first, steps, method, np.zeros((4, steps), dtype=np.float32))
    assert _lens(m, 4) == [_plen(p) + steps for p in prompts]
    m.close()
    assert toks.shape == (4, steps) and toks.dtype == np.int32 and n_out.tolist() == [steps] * 4 and amb == 0
    for b in range(4):
        assert np.array_equal(toks[b], np.asarray(want[b][1:], dtype=np.int32)), (method, b, toks[b].tolist())


@gpu
@pytest.mark.parametrize("method", [1, 2], ids=["topk", "topp"])
def test_rows_equal_their_solo_sampled_runs(method):
    """random uniform numbers, temperature 1.5: row b equals generate_sampled of sequence b alone on u01[b]; the solo runs leave the greedy ids in at least two rows, so the
    draw is exercised; every cache grows by `steps`"""
    from mllm_amd import lib
    _, _, _, prompts = _qwen2vl_case()
    steps, _ = _steps_and_u()
    first, solo = _solo(method)
    greedy = _greedy_want()
    assert first == [w[0] for w in greedy]
    assert sum(solo[b] != greedy[b][1:] for b in range(4)) >= 2
    toks, n_out, amb, lens = _b4_sampled_run(lib, method)
    assert amb == 0 and n_out.tolist() == [steps] * 4
    assert lens == [_plen(p) + steps for p in prompts]
    for b in range(4):
        assert toks[b].tolist() == solo[b], (method, b, toks[b].tolist(), solo[b])


@gpu
@pytest.mark.parametrize("key,mk", [("tlq", lambda: synth.tinyllama_tiny(mf.Q4_K)), ("qwen", synth.qwen15_tiny)], ids=["tinyllama_q4k", "qwen15"])
def test_other_configs_change_b_and_method_on_one_model(key, mk):
    """TinyLlama Q4_K (Linear head) and Qwen1.5 (tied head) on the full-range files, ONE model: B = 2 top-k, then B = 3 top-p (a second graph; row 2 starts there), then the
    greedy batch_generate for the rest -- with u01 = 0 row 0 follows the reference's 31 greedy steps through all three, rows 1 and 2 their batch-1 runs.  Then the
    sequences are prefilled again and B = 2 top-k / B = 3 top-p run on random numbers at temperature 1.5 against generate_sampled alone."""
    from mllm_amd import lib
    g = _gold("configs_tiny_fr.npz")
    cfg = mk()
    path = weights.causal_lm_file(cfg, CACHE, full_range=True)
    r = np.random.default_rng(6)
    prompts = [g[key + "_ids"]] + [r.integers(0, cfg.vocab, size=n).astype(np.int32) for n in (6, 11)]
    steps = len(g[key + "_tokens"]) - 1
    s1, s2 = 10, 10

    def alone(p, n):
        m1 = lib.Model(cfg, path)
        tok, _, _ = m1.prefill(p, want_logits=False)
        toks, _ = m1.generate(tok, n)
        m1.close()
        return [tok] + toks.tolist()
    want = [g[key + "_tokens"].tolist(), alone(prompts[1], steps), alone(prompts[2], steps - s1)]
    m = lib.Model(cfg, path)
    first = _prefill_all(m, prompts)
    assert first == [w[0] for w in want]
    t1, n1, amb, _ = m.batch_generate_sampled(first[:2], s1, 1, np.zeros((2, s1), dtype=np.float32))
    assert n1.tolist() == [s1] * 2 and amb == 0
    for b in range(2):
        assert np.array_equal(t1[b], want[b][1:s1 + 1]), (b, t1[b].tolist())
    t2, n2, amb, _ = m.batch_generate_sampled([int(t1[0][-1]), int(t1[1][-1]), first[2]], s2, 2, np.zeros((3, s2), dtype=np.float32))
    assert n2.tolist() == [s2] * 3 and amb == 0
    assert np.array_equal(t2[0], want[0][s1 + 1:s1 + s2 + 1]) and np.array_equal(t2[1], want[1][s1 + 1:s1 + s2 + 1]) and np.array_equal(t2[2], want[2][1:s2 + 1])
    rest = steps - s1 - s2
    t3, n3, _ = m.batch_generate(t2[:, -1], rest)
    assert n3.tolist() == [rest] * 3
    assert np.array_equal(t3[0], want[0][s1 + s2 + 1:]) and np.array_equal(t3[1], want[1][s1 + s2 + 1:]) and np.array_equal(t3[2], want[2][s2 + 1:s2 + rest + 1])
    assert _lens(m, 3) == [len(prompts[0]) + steps, len(prompts[1]) + steps, len(prompts[2]) + s2 + rest]
    # the draw on these heads: fresh caches, random numbers
    u = np.random.default_rng(U_SEED + 1).random((3, s1)).astype(np.float32)
    solo = {}
    for method, B in ((1, 2), (2, 3)):
        for b in range(B):
            m1 = lib.Model(cfg, path)
            tok, _, _ = m1.prefill(prompts[b], want_logits=False)
            solo[method, b], _ = m1.generate_sampled(tok, s1, method, u[b], temperature=TEMP_HOT)
            m1.close()
    for method, B in ((1, 2), (2, 3)):
        for b in range(3):
            m.batch_select(b)
            m.clear_kvcache()
        assert _prefill_all(m, prompts) == first
        t, n, amb, _ = m.batch_generate_sampled(first[:B], s1, method, u[:B], temperature=TEMP_HOT)
        assert amb == 0 and n.tolist() == [s1] * B
        for b in range(B):
            assert t[b].tolist() == solo[method, b].tolist(), (method, b)
        assert any(t[b].tolist() != want[b][1:s1 + 1] for b in range(B)), method
    m.close()


@gpu
def test_eos_stops_the_row_that_draws_it():
    """top-k on the random numbers with an eos that one row's solo run draws first at a step >= 3 and no other row draws: that row stops there (n_out, the -1 tail, its
    cache), the others finish bit-equal, and the stopped sequence carries on alone exactly as a solo run that stopped at the same id"""
    from mllm_amd import lib
    _, cfg, path, prompts = _qwen2vl_case()
    steps, u = _steps_and_u()
    first, solo = _solo(1)
    pick = None
    for b in range(4):
        for s in range(3, steps):
            e = solo[b][s]
            if e not in solo[b][:s] and all(e not in solo[o] for o in range(4) if o != b):
                pick = (b, s, e)
                break
        if pick:
            break
    assert pick is not None
    row, at, eos = pick
    m = lib.Model(cfg, path)
    assert _prefill_all(m, prompts) == first
    toks, n_out, amb, _ = m.batch_generate_sampled(first, steps, 1, u, temperature=TEMP_HOT, eos=eos)
    want_n = [at + 1 if b == row else steps for b in range(4)]
    assert amb == 0 and n_out.tolist() == want_n
    for b in range(4):
        assert toks[b][:want_n[b]].tolist() == solo[b][:want_n[b]], b
        assert np.all(toks[b][want_n[b]:] == -1), b
    assert _lens(m, 4) == [_plen(p) + n for p, n in zip(prompts, want_n)]
    m.batch_select(row)
    cont, _ = m.generate(eos, 5)
    m.close()
    p, im, me = prompts[row]
    m1 = lib.Model(cfg, path)
    tok, _, _ = m1.prefill(p, im, me, want_logits=False)
    cut, _ = m1.generate_sampled(tok, steps, 1, u[row], temperature=TEMP_HOT, eos=eos)
    assert cut.tolist() == solo[row][:at + 1]
    want_cont, _ = m1.generate(eos, 5)
    m1.close()
    assert np.array_equal(cont, want_cont)


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch
if torch.cuda.is_available():
    torch.cuda.init()
from mllm_amd import lib
import tests.test_batch_sampled as t
out = {}
for method in (1, 2):
    toks, n_out, amb, lens = t._b4_sampled_run(lib, method)
    out[str(method)] = {"toks": toks.tolist(), "n": n_out.tolist(), "amb": amb, "lens": lens}
print("RESULT " + json.dumps(out))
"""


@gpu
def test_no_graph_option_gives_the_same_ids():
    """MLLM_HIP_NO_GRAPH=1 (read once per model, so a fresh child process): the eager loop of the same step body gives the captured runs' ids for both sampled methods"""
    import json
    from mllm_amd import lib
    env = dict(os.environ, MLLM_HIP_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    for method in (1, 2):
        toks, n_out, amb, lens = _b4_sampled_run(lib, method)
        got = res[str(method)]
        assert got["toks"] == toks.tolist() and got["n"] == n_out.tolist() and got["amb"] == amb == 0 and got["lens"] == lens, method
        assert got["toks"] == _solo(method)[1], method


@gpu
def test_refusals_leave_everything_as_it_was():
    from mllm_amd import lib
    g, cfg, path, prompts = _qwen2vl_case()
    m = lib.Model(cfg, path)
    first = _prefill_all(m, prompts)
    base = [_plen(p) for p in prompts]
    u = np.zeros((4, 4), dtype=np.float32)
    bad = [dict(method=1, top_k=65), dict(method=1, temperature=0.0), dict(method=2, temperature=0.0), dict(method=2, top_p=0.0), dict(method=2, top_p=-0.5),
           dict(method=2, top_p=float("nan")), dict(method=3)]
    for kw in bad:
        with pytest.raises(lib.MllmHipError):
            m.batch_generate_sampled(first, 4, kw.pop("method"), u, **kw)
        assert _lens(m, 4) == base, kw
    with pytest.raises(lib.MllmHipError):
        m.batch_generate_sampled(first, 4, 1, None)
    assert _lens(m, 4) == base
    # the text golden's 40 ids + 57 steps pass the 96-entry cache; the other three would fit
    over = cfg.cache_limit - base[1] + 1
    with pytest.raises(lib.MllmHipError):
        m.batch_generate_sampled(first, over, 1, np.zeros((4, over), dtype=np.float32))
    assert _lens(m, 4) == base
    toks, n_out, amb, _ = m.batch_generate_sampled(first, 8, 2, np.zeros((4, 8), dtype=np.float32))          # a valid call afterwards: the right ids
    assert np.array_equal(toks[0], g["tokens"][1:9]) and np.array_equal(toks[1], g["tokens_text"][1:9]) and amb == 0
    assert _lens(m, 4) == [x + 8 for x in base]
    m.close()

"""The step-plan geometries (synth.STEP_PLAN_GEOMETRIES: causal LMs whose shapes sit at the edges of decode_step_plan's predicates) and the reference's runs on their full-range
files (tests/golden/step_plan_<id>.npz; oracle/make_golden.py --step-plan).  CPU only: the goldens are informative and small, the oracle's composed graph reproduces every
stored id and logit bit for bit, and lib.model_config hands the engine the fields it reads.  tests/test_gpu_step_plan_shapes.py replays the same files on the engine."""
import os

import numpy as np
import pytest

from mllm_amd import synth
from mllm_amd import synthfile as weights

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GIDS = list(synth.STEP_PLAN_GEOMETRIES)


def _gold(gid):
    return np.load(os.path.join(GOLD, f"step_plan_{gid}.npz"))


def test_the_table_holds_the_geometries_a_to_h():
    assert GIDS == list("ABCDEFGH")
    for gid in GIDS:
        c = synth.step_plan_geometry(gid)
        assert c.hidden % 256 == 0 and c.inter % 256 == 0 and c.hidden % c.heads == 0 and c.head_dim in (64, 128) and c.heads % c.kv_heads == 0, gid
        assert c.cache_limit == 96 and c.tie_embedding == (c.family == "qwen"), gid


@pytest.mark.parametrize("gid", GIDS)
def test_step_plan_goldens_are_informative_and_small(gid):
    """The bar of test_informative_goldens: >= 24 steps, >= 8 distinct greedy ids, an id that differs from its predecessor at >= 12 steps; at most 1,000,000 bytes a file.
    Whole logit rows for the prefill, the first three decode steps, the last step, and at least 8 steps in all."""
    g = _gold(gid)
    c = synth.step_plan_geometry(gid)
    t = g["tokens"]
    assert len(t) == synth.STEP_PLAN_STEPS >= 24
    assert len(np.unique(t)) >= 8 and int(np.count_nonzero(t[1:] != t[:-1])) >= 12, t.tolist()
    assert os.path.getsize(os.path.join(GOLD, f"step_plan_{gid}.npz")) <= 1_000_000
    steps = g["steps"].tolist()
    assert steps == list(synth.STEP_PLAN_LOGIT_STEPS) and {0, 1, 2, 3, len(t) - 1} <= set(steps) and len(steps) >= 8
    assert g["logits"].shape == (len(steps), c.vocab) and g["logits"].dtype == np.float32
    assert np.array_equal(g["logits"].argmax(axis=1), t[steps])
    assert np.array_equal(g["ids"], synth.causal_lm_ids(c, synth.STEP_PLAN_PROMPT, synth.STEP_PLAN_PROMPT_SEED[gid]))
    if "top_idx" in g.files:      # the sampled form of every step, where the vocabulary is large
        assert g["top_idx"].shape == g["top_val"].shape == (len(t), 64) and g["strided"].shape == (len(t), (c.vocab + 96) // 97)
        assert np.array_equal(g["top_idx"][:, 0], t)
        assert np.array_equal(g["top_val"][steps], np.take_along_axis(g["logits"], g["top_idx"][steps], axis=1))


@pytest.mark.parametrize("gid", GIDS)
def test_oracle_reproduces_the_step_plan_goldens(gid):
    """oracle.models.CausalLM on the geometry's full-range file: every greedy id, every stored logit (whole rows, and the sampled ones of the other steps) bit for bit."""
    from oracle import models as om
    g = _gold(gid)
    c = synth.step_plan_geometry(gid)
    m = om.CausalLM(om.Weights(weights.causal_lm_file(c, full_range=True)), c)
    kept = {int(s): i for i, s in enumerate(g["steps"])}
    cur = g["ids"]
    for s, want in enumerate(g["tokens"]):
        lg = m.forward(cur)
        assert int(np.argmax(lg)) == int(want), (s, int(np.argmax(lg)), int(want))
        if s in kept:
            assert np.array_equal(lg, g["logits"][kept[s]]), (s, float(np.abs(lg - g["logits"][kept[s]]).max()))
        if "top_idx" in g.files:
            assert np.array_equal(lg[g["top_idx"][s]], g["top_val"][s]) and np.array_equal(lg[::97], g["strided"][s]), s
        cur = [int(want)]


@pytest.mark.parametrize("gid", GIDS)
def test_model_config_maps_the_step_plan_geometries(gid):
    from mllm_amd import lib
    c = synth.step_plan_geometry(gid)
    cc = lib.model_config(c)
    assert (cc.hidden, cc.inter, cc.layers, cc.heads, cc.kv_heads, cc.vocab, cc.cache_limit) == (c.hidden, c.inter, c.layers, c.heads, c.kv_heads, c.vocab, 96)
    qwen = c.family == "qwen"
    assert (cc.arch, cc.tie_embedding, cc.qkv_bias) == ((lib.ARCH_QWEN, 1, 1) if qwen else (lib.ARCH_LLAMA, 0, 0))
    assert cc.rope_theta == (1000000.0 if qwen else 10000.0) and cc.rms_eps == np.float32(1e-6) and cc.final_eps == np.float32(1e-6)
    assert lib.model_config(c, cache_limit=2049).cache_limit == 2049


def test_model_config_carries_the_cache_limit_of_geometry_i():
    """Geometry I is the toy Qwen2-VL at cache_limit 2048 and 2049 (the last limit with the pipelined attention and the merged launches, and the first without)."""
    from mllm_amd import lib
    c = synth.qwen2vl_tiny()
    assert [lib.model_config(c, cache_limit=n).cache_limit for n in (2048, 2049)] == [2048, 2049] and lib.model_config(c).cache_limit == 96

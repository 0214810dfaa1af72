"""Every launch form of the decode step at the edges of its shape predicate (decode_step_plan, csrc/kernels_decode.hip).  The geometries are synth.STEP_PLAN_GEOMETRIES (A .. H:
each sits at, or just across, one edge; DESIGN.md "Step-plan geometries" has the table) plus I, the toy Qwen2-VL at cache_limit 2048 and 2049.  The yardstick is the
reference's own run on each geometry's full-range file (tests/golden/step_plan_<id>.npz: greedy ids that change from step to step, whole logit rows): ids ==, logits
np.array_equal, no tolerance.  Which launches a step makes is asserted against the literal dicts below, written from the predicates by hand -- never asked of the library."""
import contextlib
import os

import numpy as np
import pytest

from mllm_amd import synth
from mllm_amd import synthfile as weights

pytestmark = pytest.mark.gpu
CACHE = os.environ.get("MLLM_AMD_CACHE", "/tmp/mllm_amd_cache")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# launches per step and kind of the three plans a model of L layers can get (the ALTERNATIVES' plans; PLAN spells its dicts out).  CHAIN: layer 0's q|k|v and attention (+ o-projection) on their own, every layer's gate|up, a chain launch (down + the next layer's
# q|k|v + attention + o-projection) behind every layer but the last, whose down projection is a launch of its own.  FRONT: the same without the down projection in the shared
# launch.  FIVE: q|k|v, attention, o-projection, gate|up, down for every layer.
def _chain(L): return {"qkv": 1, "attn": 1, "gateup": L, "chain": L - 1, "down": 1, "head": 1, "next": 1}
def _front(L): return {"qkv": 1, "attn": 1, "front": L - 1, "gateup": L, "down": L, "head": 1, "next": 1}
def _five(L): return {"qkv": L, "attn": L, "o_proj": L, "gateup": L, "down": L, "head": 1, "next": 1}


PLAN = {
    "A": {"qkv": 1, "attn": 1, "gateup": 3, "chain": 2, "down": 1, "head": 1, "next": 1},      # heads * D = H = 2048 still merges; 22 super-blocks per down row
    "B": {"qkv": 1, "attn": 1, "gateup": 3, "chain": 2, "down": 1, "head": 1, "next": 1},      # 17 super-blocks: the first the lane-per-super-block down projection serves
    "C": {"qkv": 1, "attn": 1, "gateup": 3, "chain": 2, "down": 1, "head": 1, "next": 1},      # 40 super-blocks: the last
    "D": {"qkv": 1, "attn": 1, "front": 2, "gateup": 3, "down": 3, "head": 1, "next": 1},      # 41: no chain launch
    "E": {"qkv": 1, "attn": 1, "gateup": 3, "chain": 2, "down": 1, "head": 1, "next": 1},      # D = 64, 19 super-blocks
    "F": {"qkv": 3, "attn": 3, "o_proj": 3, "gateup": 3, "down": 3, "head": 1, "next": 1},     # heads * D = 2304 > 2048: nothing merges
    "G": {"qkv": 2, "attn": 2, "o_proj": 2, "gateup": 2, "down": 2, "head": 1, "next": 1},     # 2 layers of H = 4096 (the fused tied head's LDS does not fit there: before the plan asked, the first decode step was refused)
    "H": {"qkv": 1, "attn": 1, "front": 2, "gateup": 3, "down": 3, "head": 1, "next": 1},      # down rows of 5 super-blocks: below pjb_serves, no chain launch
}

# time_step does not tell blk, cont, persist or the head form apart.  Where one of those is a geometry's point, the same file also runs with the option that takes the other
# form (and the launches that option gives): both must give the reference's ids and logits, so a wrong form cannot hide behind a right one.
ALTERNATIVES = [
    ("A", {"merge_o": 3}, _front(3)),                        # the chain launch's roles as front launches + the lane-per-super-block down projection on its own
    ("B", {"chain_cont": 0}, _chain(3)),                     # q|k|v role on workgroups of its own (default: carried on by the down role's)
    ("B", {"no_pjb": 1}, _front(3)),                         # 17 super-blocks on the eight-lane down projection
    ("C", {"chain_cont": 0}, _chain(3)),
    ("C", {"no_pjb": 1}, _front(3)),                         # 40 super-blocks on the eight-lane down projection (NS = 5)
    ("C", {"no_gub": 1}, _chain(3)),                         # gate|up of 5 super-blocks per row on the eight-lane kernel
    ("E", {"chain_cont": 0}, _chain(3)),
    ("E", {"no_pjb": 1}, _front(3)),
    ("F", {"no_pjb": 1}, _five(3)),                          # 25 super-blocks on the eight-lane down projection (NS = 4)
    ("F", {"gu_persist": 0}, _five(3)),                      # gate|up a workgroup per row group (default at NS = 2: two walking workgroups per CU)
    ("G", {"gu_persist": 0, "qkv_persist": 0}, _five(2)),    # neither walks
    ("H", {"qkv_persist": 0}, _front(3)),                    # the Linear head a workgroup per row group (1025 workgroups)
    ("H", {"no_gub": 1}, _front(3)),
]


@contextlib.contextmanager
def _options(lib, opts):
    try:
        for k, v in opts.items():
            lib.set_option(k, v)
        yield
    finally:
        for k in opts:
            lib.set_option(k, -1)


def _case(gid):
    cfg = synth.step_plan_geometry(gid)
    return np.load(os.path.join(GOLD, f"step_plan_{gid}.npz")), cfg, weights.causal_lm_file(cfg, CACHE, full_range=True)


def _check_row(g, s, lg):
    """step s's logits against everything the golden holds of that step"""
    kept = g["steps"].tolist()
    if s in kept:
        want = g["logits"][kept.index(s)]
        assert np.array_equal(lg, want), (s, float(np.abs(lg - want).max()), int(np.count_nonzero(lg != want)))
    if "top_idx" in g.files:
        assert np.array_equal(lg[g["top_idx"][s]], g["top_val"][s]) and np.array_equal(lg[::97], g["strided"][s]), s


def _stepwise(m, g):
    """prefill, then one decode call per step (each a replay of the captured step): every id, every stored logit"""
    want = g["tokens"].tolist()
    tok, lg, _ = m.prefill(g["ids"])
    got = [tok]
    _check_row(g, 0, lg)
    for s in range(1, len(want)):
        tok, lg, _ = m.decode(tok)
        got.append(tok)
        _check_row(g, s, lg)
    assert got == want, (got, want)


def _eager_step_and_hand_back(m, g, plan, at=7, eager=9):
    """`at` graph steps, `eager` steps launch by launch (time_step), one more graph step: the launches of a step are `plan`, the ids the golden's throughout"""
    want = g["tokens"].tolist()
    m.clear_kvcache()
    tok, _, _ = m.prefill(g["ids"], want_logits=False)
    gen, _ = m.generate(tok, at)
    assert [tok] + gen.tolist() == want[:at + 1]
    kinds, last = m.time_step(int(gen[-1]), eager)
    print("launches per step:", {k: n for k, (_, n) in kinds.items()})
    assert {k: n for k, (_, n) in kinds.items()} == plan
    assert last == want[at + eager]
    tok, lg, _ = m.decode(last)
    assert tok == want[at + eager + 1]
    _check_row(g, at + eager + 1, lg)


@pytest.mark.parametrize("gid", list(PLAN))
def test_geometry_reproduces_the_reference_on_the_derived_plan(gid):
    from mllm_amd import lib
    g, cfg, path = _case(gid)
    want = g["tokens"].tolist()
    m = lib.Model(cfg, path)
    try:
        _stepwise(m, g)
        m.clear_kvcache()      # the captured graph over the whole run
        tok, _, _ = m.prefill(g["ids"], want_logits=False)
        gen, _ = m.generate(tok, len(want) - 1)
        assert [tok] + gen.tolist() == want
        _eager_step_and_hand_back(m, g, PLAN[gid])
    finally:
        m.close()


@pytest.mark.parametrize("gid,opts,plan", ALTERNATIVES, ids=[f"{g}-" + "-".join(f"{k}{v}" for k, v in o.items()) for g, o, _ in ALTERNATIVES])
def test_geometry_on_the_other_form_gives_the_same_run(gid, opts, plan):
    from mllm_amd import lib
    g, cfg, path = _case(gid)
    with _options(lib, opts):
        m = lib.Model(cfg, path)      # the options are read once, when the model is created
        try:
            _stepwise(m, g)
            _eager_step_and_hand_back(m, g, plan)
        finally:
            m.close()


def test_cache_limit_2048_merges_and_2049_does_not():
    """Geometry I: the toy Qwen2-VL at cache_limit 2048 (the last with the pipelined attention: the o-projection rides in layer 0's attention launch, layer 1 is a front launch)
    and at 2049 (five launches per layer).  The reference's text run does not depend on the limit: 40 ids and every logit, both ways."""
    from mllm_amd import lib
    g = np.load(os.path.join(GOLD, "qwen2vl_tiny_fr.npz"))
    cfg = synth.qwen2vl_tiny()
    path = weights.qwen2vl_file(cfg, CACHE, full_range=True)
    want = g["tokens_text"].tolist()
    plans = {2048: {"qkv": 1, "attn": 1, "front": 1, "gateup": 2, "down": 2, "head": 1, "next": 1},
             2049: {"qkv": 2, "attn": 2, "o_proj": 2, "gateup": 2, "down": 2, "head": 1, "next": 1}}
    for limit, plan in plans.items():
        m = lib.Model(cfg, path, cache_limit=limit)
        try:
            tok, lg, _ = m.prefill(g["ids_text"])
            got, rows = [tok], [lg]
            for _ in range(1, 24):
                tok, lg, _ = m.decode(tok)
                got.append(tok)
                rows.append(lg)
            assert got == want[:24], (limit, got)
            assert np.array_equal(np.stack(rows), g["logits_text"][:24]), limit
            kinds, last = m.time_step(tok, 9)
            assert {k: n for k, (_, n) in kinds.items()} == plan, limit
            assert last == want[32], limit
            for s in range(33, 40):      # the graph replay carries on from the eager steps' state
                last, lg, _ = m.decode(last)
                assert last == want[s] and np.array_equal(lg, g["logits_text"][s]), (limit, s)
        finally:
            m.close()


@pytest.mark.parametrize("gid", ["A", "E"])
def test_batch_generate_b2_rows_equal_the_batch1_ids(gid):
    """B = 2 on a chain-launch geometry with D = 128 (A) and D = 64 (E): row 0 is the golden prompt (the reference's ids), row 1 a 9-id prompt against its batch-1 run.
    Down rows of 22 and 19 super-blocks: the M > 1 GEMV once chose its weight blocks by flags of activation planes it had not loaded yet, and both rows were wrong."""
    from mllm_amd import lib
    g, cfg, path = _case(gid)
    steps = len(g["tokens"]) - 1
    other = np.random.default_rng(5).integers(0, cfg.vocab, size=9).astype(np.int32)
    m = lib.Model(cfg, path)
    try:
        tok, _, _ = m.prefill(other, want_logits=False)
        gen, _ = m.generate(tok, steps)
        alone = [tok] + gen.tolist()
    finally:
        m.close()
    m = lib.Model(cfg, path)
    try:
        m.batch_begin(2)
        first = []
        for b, p in enumerate((g["ids"], other)):
            m.batch_select(b)
            first.append(m.prefill(p, want_logits=False)[0])
        assert first == [int(g["tokens"][0]), alone[0]]
        toks, n_out, _ = m.batch_generate(first, steps)
        assert n_out.tolist() == [steps, steps]
        assert np.array_equal(toks[0], g["tokens"][1:]), toks[0].tolist()
        assert np.array_equal(toks[1], np.asarray(alone[1:], dtype=np.int32)), toks[1].tolist()
    finally:
        m.close()

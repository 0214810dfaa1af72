"""Every prefill attention instance, pitch and tile edge at op level: each (D, K/V type, causal) cell of mllm_hip_fa2 and mllm_hip_fa2_vt (csrc/kernels_attn.hip:
fa2_prefill_kernel and the launch_fa2 routing around it) launched through the C ABI at the smallest shapes that reach the edges of its tiling -- FA_R = 32 query rows per
workgroup, key chunks of FA_KCH = 32, the causal cut of the chunk walk, partial row tiles on the diagonal, the fp16 leftover rule, the head / row-block remap, the
one-launch-per-row route of Sq in {2, 3} and the batch form.  The case lists and the seeded inputs live in tests/attn_forms_table.py; tests/test_attn_forms_host.py holds that
table against the launchers' source.

Bar: every comparison is against oracle.attention on the same values, on the bit patterns (uint32 views; a position where both sides are NaN counts as equal, a NaN on one
side only does not).  No tolerance anywhere.  Every operand is pitched the way the engine pitches it (ops.flash_attention2_pitched and its kin): Q inside a q|k|v buffer, K / V
rows that go on past Hkv D, guard rows behind every operand.  Every element the op does not own holds NaN -- one read of it makes an output row NaN -- except the columns
>= Sk of the transposed V slab, which the kernels read by design (include/mllm_hip.h): those hold the largest finite fp16.  The output's pad columns and guard rows must still
hold the sentinel afterwards, as must the whole output of a refused call."""
import functools

import numpy as np
import pytest

from tests import attn_forms_table as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mllm_amd import lib, ops  # noqa: E402
from oracle import oracle as orc  # noqa: E402

F16_MAX = 65504.0      # 0x7BFF


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    ops.require_gpu()


def _u16(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


def oracle(q, k, v, Sq, Sk, Hq, Hkv, D, causal):
    return orc.attention(q, _u16(k), _u16(v), Sq, Sk, Hq, Hkv, D, causal)


@functools.lru_cache(maxsize=None)
def inputs(tag, Sq, Sk, Hq, Hkv, D, f16):
    arrs = T.qkv(tag, Sq, Sk, Hq, Hkv, D, f16)
    for a in arrs:
        a.setflags(write=False)
    return arrs


def assert_bits(o, ref, what):
    """Rows 0 .. Sq-1, columns 0 .. Hq D - 1 of the device output `[Sq + guard rows][ldo]` equal `ref` bit for bit (NaN against NaN is equal), everything else is sentinel."""
    Sq, n = ref.shape
    got = o.detach().cpu().numpy()
    g, r = got[:Sq, :n], ref
    both_nan = np.isnan(g) & np.isnan(r)
    bad = np.argwhere((g.view(np.uint32) != r.view(np.uint32)) & ~both_nan)
    assert bad.size == 0, (what, f"{len(bad)} of {r.size} differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]!r} != {r[tuple(bad[0])]!r}")
    s = ops.is_sentinel(o)
    assert s[:Sq, n:].all() and s[Sq:].all(), (what, "pad columns or guard rows written")


def launch(form, q, k, v, Sq, Sk, Hq, Hkv, D, causal, **kw):
    ldq, ldk, ldv, ldo = T.pitches(Hq, Hkv, D)
    if form == T.VT:
        ldvt = kw.pop("ldvt", ((Sk + 63) // 64) * 64 + 128)      # the engine's pitch unless the case is about the pitch
        return ops.flash_attention2_vt_pitched(q, k, v, Sq, Sk, Hq, Hkv, D, causal, ldq, ldk, ldvt, ldo, **kw)
    return ops.flash_attention2_pitched(q, k, v, Sq, Sk, Hq, Hkv, D, causal, ldq, ldk, ldv, ldo, **kw)


def run(cell, Sq, Sk, heads=None, arrs=None, tag="m"):
    """One case of `cell` against the oracle.  The transposed slab runs twice, its read-by-design pad columns holding the largest finite fp16 and zero: same bits."""
    form, D, f16, causal = cell
    Hq, Hkv = heads or T.heads_of(D)
    q, k, v = arrs if arrs is not None else inputs(tag, Sq, Sk, Hq, Hkv, D, f16)
    ref = oracle(q, k, v, Sq, Sk, Hq, Hkv, D, causal)
    what = (T.cell_id(cell), Sq, Sk, Hq, Hkv)
    if form == T.VT:
        o = launch(form, q, k, v, Sq, Sk, Hq, Hkv, D, causal, vt_pad=F16_MAX)
        assert_bits(o, ref, what + ("pad = max fp16",))
        assert_bits(launch(form, q, k, v, Sq, Sk, Hq, Hkv, D, causal, vt_pad=0.0), ref, what + ("pad = 0",))
    else:
        assert_bits(launch(form, q, k, v, Sq, Sk, Hq, Hkv, D, causal), ref, what)
    return ref


cells = pytest.mark.parametrize("cell", T.CELLS, ids=T.cell_id)


# ---- the matrix -------------------------------------------------------------------------------------------------------------------------------------------------------------
@cells
def test_square_shapes_on_row_block_and_chunk_edges(cell):
    for S in T.SQUARE:
        ref = run(cell, S, S)
        assert np.isfinite(ref).all()


@cells
def test_short_query_block_under_chunk_edges(cell):
    for Sk in T.SHORT_SK:
        run(cell, T.SHORT_SQ, Sk)


@pytest.mark.parametrize("cell", T.CAUSAL_CELLS, ids=T.cell_id)
def test_causal_cut_of_the_chunk_walk_around_a_chunk_boundary(cell):
    for Sk in T.KLIM_SK:
        run(cell, T.KLIM_SQ, Sk)


@pytest.mark.parametrize("cell", T.F16_CELLS, ids=T.cell_id)
def test_fp16_leftover_rule_ignores_the_dropped_keys(cell):
    _, D, _, _ = cell
    for Sq in T.F16_LEFT_SQ:
        for Sk in T.F16_LEFT_SK:
            Hq, Hkv, q, k, v = T.f16_left_case(Sq, Sk, D)
            run(cell, Sq, Sk, heads=(Hq, Hkv), arrs=(q, k, v))


@pytest.mark.parametrize("cell", T.CAUSAL_CELLS, ids=T.cell_id)
def test_causal_with_more_queries_than_keys(cell):
    for Sq, Sk in T.NEG_DELTA:
        ref = run(cell, Sq, Sk)
        if Sq - Sk >= 4:      # the reference's literal reading: the first row tile has no live key tile, 0 * (1 / 0)
            assert np.isnan(ref[:4]).all() and np.isfinite(ref[4:]).all()
        else:
            assert np.isfinite(ref).all()


@cells
def test_two_and_three_rows_take_one_decode_launch_each(cell):
    for Sq in T.TINY_SQ:
        for Sk in T.tiny_sk(Sq):
            run(cell, Sq, Sk)


@pytest.mark.parametrize("D", T.FA2_D)
def test_online_softmax_rescale(D):
    for spike in T.RESCALE_LITERAL_SPIKES:
        run((T.ROWS, D, True, True), T.RESCALE_S, T.RESCALE_S, heads=(1, 1), arrs=T.rescale_literal_case(D, spike))
    for spike in T.RESCALE_STEPPED_SPIKES:
        for form in (T.ROWS,) + ((T.VT,) if D in T.FA2_VT_D else ()):
            run((form, D, True, False), T.SHORT_SQ, T.RESCALE_S, heads=(1, 1), arrs=T.rescale_stepped_case(D, spike))


# ---- once per D ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", T.FA2_D)
def test_head_remap_and_groups(D):
    forms = [(T.ROWS, False), (T.ROWS, True)] + ([(T.VT, True)] if D in T.FA2_VT_D else [])
    for Hq, Hkv in T.HEADS:
        for form, f16 in forms:
            run((form, D, f16, True), T.HEADS_S, T.HEADS_S, heads=(Hq, Hkv), tag="heads")


@pytest.mark.parametrize("D", T.FA2_D)
def test_batch_form_every_set_against_the_oracle(D):
    nb, Sq = T.BATCH_NB, T.BATCH_SQ
    Hq, Hkv = T.heads_of(D)
    ldq, ldk, ldv, ldo = T.pitches(Hq, Hkv, D)
    for Sk in T.BATCH_SK:
        for f16 in (False, True):
            sets = [inputs(("batch", b), Sq, Sk, Hq, Hkv, D, f16) for b in range(nb)]
            q, k, v = (np.stack([s[i] for s in sets]) for i in range(3))
            for causal in (False, True):
                o = ops.flash_attention2_batch_pitched(q, k, v, Sq, Sk, Hq, Hkv, D, causal, ldq, ldk, ldv, ldo)
                for b in range(nb):
                    assert_bits(o[b], oracle(q[b], k[b], v[b], Sq, Sk, Hq, Hkv, D, causal), (D, Sk, f16, causal, b))


def refused(call, o, what):
    with pytest.raises(lib.MllmHipError, match=r"code %d\b" % lib.ERR_SHAPE):
        call()
    torch.cuda.synchronize()
    assert ops.is_sentinel(o).all(), (what, "a refused call wrote to its output")


def test_batch_form_refuses_fewer_than_four_rows():
    D, Sk, nb = 64, 9, 3
    Hq, Hkv = T.heads_of(D)
    ldq, ldk, ldv, ldo = T.pitches(Hq, Hkv, D)
    for Sq in (1, 2, 3):
        sets = [inputs(("batch", b), Sq, Sk, Hq, Hkv, D, True) for b in range(nb)]
        q, k, v = (np.stack([s[i] for s in sets]) for i in range(3))
        o = ops.sentinel_out(nb * (Sq + 2), ldo)
        refused(lambda: ops.flash_attention2_batch_pitched(q, k, v, Sq, Sk, Hq, Hkv, D, True, ldq, ldk, ldv, ldo, out=o), o, Sq)


# ---- the transposed slab's pitch: accepted exactly at the bound (the guard rows behind the slab hold NaN: a read past the last row's ldvt columns would show), refused 8 below --
@pytest.mark.parametrize("D", T.FA2_VT_D)
@pytest.mark.parametrize("Sq,Sk", [(8, 33), (33, 65), (5, 7), (4, 32), (1, 33), (1, 129), (3, 8), (2, 130)])
def test_transposed_slab_pitch_bound(D, Sq, Sk):
    Hq, Hkv = T.heads_of(D)
    bound = T.vt_min_ld(Sq, Sk)
    assert bound % 8 == 0 and bound >= Sk
    q, k, v = inputs("vtld", Sq, Sk, Hq, Hkv, D, True)
    for causal in (False, True):
        ref = oracle(q, k, v, Sq, Sk, Hq, Hkv, D, causal)
        for pad in (F16_MAX, 0.0):
            assert_bits(launch(T.VT, q, k, v, Sq, Sk, Hq, Hkv, D, causal, ldvt=bound, vt_pad=pad), ref, (D, Sq, Sk, causal, pad))
        if bound - 8 >= Sk:      # (below Sk the harness has no slab to build; the entry's check does not depend on it)
            o = ops.sentinel_out(Sq + 2, T.pitches(Hq, Hkv, D)[3])
            refused(lambda: launch(T.VT, q, k, v, Sq, Sk, Hq, Hkv, D, causal, ldvt=bound - 8, out=o), o, (D, Sq, Sk, causal))

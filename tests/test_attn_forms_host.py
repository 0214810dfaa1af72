"""CPU side of tests/test_gpu_attn_forms.py.  (1) Its case table (tests/attn_forms_table.py) is held against the source of csrc/kernels_attn.hip: the FA2_CASE lists of
mllm_hip_fa2 / mllm_hip_fa2_batch, the K/V types each case instantiates, mllm_hip_fa2_vt's switch, the tile constants FA_R / FA_KCH / FA_VCH and the rules the table restates
(sk_eff, klim, the head remap, the slab pitch bound) are read out of the text -- a new instance or a changed tile size fails here until the table follows.  (2) The edges the
table claims are derived again from those constants.  (3) On the oracle alone: the constructed inputs do what the cases say -- the keys the fp16 rule drops would move every
output if read, and the stepped rescale case moves every row's maximum at key 0 and at the spiked key only.  (4) The engine's and ops.flash_attention2_vt's slab pitches
satisfy mllm_hip_fa2_vt's bound, from their formulas.  No GPU."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import attn_forms_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mllm_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _between(text, start, end):
    body = text[text.index(start):]
    return body[:body.index(end)]


def test_table_lists_every_instance():
    text = _src("kernels_attn.hip")
    for entry in ('extern "C" int mllm_hip_fa2(', 'extern "C" int mllm_hip_fa2_batch('):
        body = _between(text, entry, "#undef FA2_CASE")
        assert sorted(int(d) for d in re.findall(r"\bFA2_CASE\((\d+)\)", body)) == sorted(T.FA2_D), entry
        assert "launch_fa2<DD, true>(" in body and "launch_fa2<DD, false>(" in body, entry      # every case: fp16 and fp32 K/V
    vt = _between(text, 'extern "C" int mllm_hip_fa2_vt(', "\n}")
    got = re.findall(r"case (\d+): return launch_fa2<(\d+), true, true>\(", vt)
    assert got and all(a == b for a, b in got) and sorted(int(a) for a, _ in got) == sorted(T.FA2_VT_D), got
    assert len(T.CELLS) == len(set(T.CELLS)) == 4 * len(T.FA2_D) + 2 * len(T.FA2_VT_D)
    assert {(f, D, h) for f, D, h, _ in T.CELLS} == {(T.ROWS, D, h) for D in T.FA2_D for h in (False, True)} | {(T.VT, D, True) for D in T.FA2_VT_D}
    assert all((f, D, h, c) in T.CELLS for f, D, h, _ in T.CELLS for c in (False, True))


def test_tile_constants_and_rules_are_the_ones_the_table_restates():
    text, core = _src("kernels_attn.hip"), _src("kernels_attn_core.h")
    assert "constexpr int FA_R = %d, FA_KCH = %d;" % (T.FA_R, T.FA_KCH) in text
    assert "constexpr int FA_VCH = %d;" % T.FA_VCH in core
    assert "const int left = F16 ? (Tc ? Sk % Tc : 0) : Sk % 4;" in text and "const int sk_eff = Tc * 4 + left;" in text      # T.sk_eff
    assert "if (causal) klim = min(sk_eff, r0 + FA_R + delta + 4);" in text                                                     # T.klim
    assert "if ((Hq & 7) == 0) {" in text                                                                                       # the remap T.HEADS is about
    assert "if (Sq == 1) return decode_row(" in text and "if (Sq < 4) {" in text                                                # the routes of Sq = 1 and Sq in {2, 3}
    assert "const int64_t unit = Sq >= 4 ? FA_KCH : FA_VCH;" in text and "if (ldvt < fa2_vt_min_ld(Sq, Sk)) return MLLM_HIP_ERR_SHAPE;" in text      # T.vt_min_ld


def test_edges_follow_from_the_constants():
    R, KC = T.FA_R, T.FA_KCH
    assert T.SQUARE == [4, 5, 31, 32, 33, 65] and T.SHORT_SQ == 8 and T.SHORT_SK == [31, 32, 33, 63, 64, 65, 97]
    assert {R - 1, R, R + 1} <= set(T.SQUARE) and {KC - 1, KC, KC + 1, 2 * KC - 1, 2 * KC, 2 * KC + 1} <= set(T.SHORT_SK)
    assert any(S > 2 * R for S in T.SQUARE)                                         # three row blocks
    assert sum(S % 4 == 1 for S in T.SQUARE) >= 3                                   # a last row tile of one row, on the diagonal when causal (Sq = Sk)
    # the causal cut: never met by (b), met inside a chunk by (a)'s largest shape, and around a chunk boundary by KLIM_SK
    for f16 in (False, True):
        for Sk in T.SHORT_SK:
            assert T.klim(0, T.SHORT_SQ, Sk, f16, True) == T.sk_eff(Sk, f16) == Sk
        S = T.SQUARE[-1]
        assert T.klim(0, S, S, f16, True) == R + 4 and KC < R + 4 < 2 * KC
        assert [T.klim(0, T.KLIM_SQ, Sk, f16, True) for Sk in T.KLIM_SK] == [2 * KC - 1, 2 * KC, 2 * KC + 1]
        assert all(T.klim(R, T.KLIM_SQ, Sk, f16, True) == Sk for Sk in T.KLIM_SK)   # the last row block walks every key
    # the fp16 leftover rule differs from Sk % 4 exactly where the table says, by the amounts it says
    drops = {Sk: T.sk_eff(Sk, True) for Sk in range(1, 4096) if T.sk_eff(Sk, True) != T.sk_eff(Sk, False) and Sk >= 4}
    assert drops == T.F16_LEFT_DROPS == {5: 4, 6: 4, 7: 4, 10: 8, 11: 9, 15: 12}
    assert all(T.sk_eff(Sk, False) == Sk for Sk in range(1, 4096))
    assert set(drops) <= set(T.F16_LEFT_SK) and {Sk - 1 for Sk in drops} | {Sk + 1 for Sk in drops} <= set(T.F16_LEFT_SK)
    assert T.NEG_DELTA == [(8, 7), (12, 8)] and any(Sq - Sk >= 4 for Sq, Sk in T.NEG_DELTA)      # a whole row tile without a live key tile
    assert T.TINY_SQ == (2, 3) and all(T.tiny_sk(Sq) == (Sq, Sq + 5) for Sq in T.TINY_SQ)
    assert all(KC <= s < T.RESCALE_S for s in T.RESCALE_LITERAL_SPIKES + T.RESCALE_STEPPED_SPIKES)
    assert any(s % KC == 0 for s in T.RESCALE_LITERAL_SPIKES) and any(s % KC == 0 for s in T.RESCALE_STEPPED_SPIKES)      # tile 0 of a chunk: the carried maximum
    assert any(s >= 2 * KC and s % KC >= 4 for s in T.RESCALE_STEPPED_SPIKES)                                            # behind a whole chunk without a move
    assert [h for h in T.HEADS if h[0] % 8 == 0 and h[0] == h[1]] and [h for h in T.HEADS if h[0] % 8 == 0 and h[0] == 4 * h[1]]
    assert [h for h in T.HEADS if h[0] % 8 and h[0] > h[1]] and (1, 1) in T.HEADS and T.HEADS_S > 2 * R
    assert T.BATCH_NB == 3 and T.BATCH_SQ == 33 and T.BATCH_SK == (33, 40)
    for D in T.FA2_D:
        Hq, Hkv = T.heads_of(D)
        ldq, ldk, ldv, ldo = T.pitches(Hq, Hkv, D)
        assert Hq in (2, 4) and ldq == (Hq + 2 * Hkv) * D and ldk == Hkv * D + 8 and ldv % 8 == 0 and ldv > Hkv * D and ldo > Hq * D


def test_slab_pitches_in_use_satisfy_the_bound():
    """mllm_hip_fa2_vt asks for ldvt >= Sk rounded up to 32 (Sq >= 4) or 128 (Sq < 4), so at most round128(Sk) <= Sk + 127.  The engine pitches its slab at
    round64(T) + 128 >= T + 128 for a cache of T rows and calls with Sk <= T; ops.flash_attention2_vt uses round64(Sk) + 128 >= Sk + 128.  Both exceed Sk + 127."""
    assert "m->vt_ld = ((T + 63) & ~63) + 128;" in _src("engine.hip")
    assert "ld = ((Sk + 63) // 64) * 64 + 128 " in open(os.path.join(ROOT, "mllm_amd", "ops.py")).read()
    for Sk in list(range(1, 1300)) + [32768, 32769]:
        for Sq in (1, 3, 4, 100):
            b = T.vt_min_ld(Sq, Sk)
            assert Sk <= b <= Sk + 127 and b % 8 == 0 and (b - Sk < 32 or Sq < 4)
            assert ((Sk + 63) & ~63) + 128 >= Sk + 128 > b
    header = open(os.path.join(ROOT, "include", "mllm_hip.h")).read()
    doc = header[:header.index("int mllm_hip_fa2_vt(")][-1400:]
    assert "multiple of 32" in doc and "multiple of 128" in doc and "FINITE" in doc and "MLLM_HIP_ERR_SHAPE" in doc and "zero-fills" in doc


def _changed(a, b):
    return float(np.mean(a.view(np.uint32) != b.view(np.uint32)))


@pytest.mark.parametrize("D", T.FA2_D)
def test_dropped_keys_would_move_every_output(D):
    """(c): on the oracle, the fp16 rule's result (keys sk_eff .. Sk - 1 ignored) against the fp32 rule's on the same values (every key read), not causal."""
    for Sq in T.F16_LEFT_SQ:
        for Sk, eff in T.F16_LEFT_DROPS.items():
            Hq, Hkv, q, k, v = T.f16_left_case(Sq, Sk, D)
            assert np.isfinite(k.astype(np.float32)).all() and np.isfinite(v.astype(np.float32)).all()
            kept = orc.attention(q, k.view(np.uint16), v.view(np.uint16), Sq, Sk, Hq, Hkv, D, False)
            read = orc.attention(q, k.astype(np.float32), v.astype(np.float32), Sq, Sk, Hq, Hkv, D, False)
            only = orc.attention(q, k[:eff].view(np.uint16), v[:eff].view(np.uint16), Sq, eff, Hq, Hkv, D, False)
            assert np.isfinite(kept).all() and _changed(kept, read) >= 0.99, (D, Sq, Sk)
            assert np.array_equal(kept.view(np.uint32), only.view(np.uint32)), (D, Sq, Sk)      # the rule is "the first sk_eff keys"


@pytest.mark.parametrize("D", T.FA2_D)
def test_stepped_rescale_case_moves_the_maximum_where_it_says(D):
    for spike in T.RESCALE_STEPPED_SPIKES:
        q, k, v = T.rescale_stepped_case(D, spike)
        s = q.astype(np.float64) @ k.astype(np.float64).T / np.sqrt(D)                    # [8][96]
        run_max = np.maximum.accumulate(s, axis=1)
        moved = np.diff(run_max, axis=1) > 0
        assert moved[:, spike - 1].all() and moved.sum() == moved.shape[0], (D, spike)    # one move per row behind key 0: at the spiked key
        assert (s[:, 0] > 5).all() and (s[:, spike] > 25).all() and np.abs(np.delete(s, [0, spike], axis=1)).max() < 2
    for spike in T.RESCALE_LITERAL_SPIKES:
        q, k, v = T.rescale_literal_case(D, spike)
        s = q[-1].astype(np.float64) @ k.astype(np.float64).T / np.sqrt(D)
        assert np.argmax(s) == spike and s[spike] > np.delete(s, spike).max() + 2, (D, spike)      # the last row's maximum jumps at the spiked key

"""The attention instances, pitches and tile edges tests/test_gpu_attn_forms.py launches, as data: every (D, K/V type, causal) cell of mllm_hip_fa2 and mllm_hip_fa2_vt
(csrc/kernels_attn.hip), the shapes that sit on the edges of fa2_prefill_kernel's tiling, and the seeded inputs of every case.  Importable without torch or a GPU:
tests/test_attn_forms_host.py reads the launchers' instance lists and tile constants out of the source and holds this table against them, and checks on the oracle alone that
the constructed inputs (the spiked keys) do what the cases say they do.

The rules below restate the launcher and the kernel by hand (they are never asked of the library):
  launch_fa2              Sq == 1: one decode launch; Sq in {2, 3}: Br = Bc = 1, one decode launch per row; Sq >= 4: fa2_prefill_kernel, FA_R query rows per workgroup,
                          key chunks of FA_KCH
  sk_eff                  the key columns the reference's tiling walks: Tc = Sk / 4, 4 Tc + Sk % 4 for fp32 K/V, 4 Tc + Sk % Tc for fp16 K/V
  klim                    causal: the row block at r0 walks chunks below min(sk_eff, r0 + FA_R + (Sk - Sq) + 4)
  mllm_hip_fa2_vt         ldvt >= Sk rounded up to FA_KCH (Sq >= 4) or to FA_VCH (Sq < 4)
"""
import zlib

import numpy as np

FA_R, FA_KCH, FA_VCH = 32, 32, 128          # the constants every edge below was derived from (held against the source by the host test)

# ---- the instances ------------------------------------------------------------------------------------------------------------------------------------------------------
FA2_D = (16, 64, 80, 128)                   # mllm_hip_fa2 / mllm_hip_fa2_batch: FA2_CASE(D), each with fp32 and fp16 K/V
FA2_VT_D = (64, 128)                        # mllm_hip_fa2_vt's switch
ROWS, VT = "rows", "vt"                     # K/V as rows [Sk][Hkv D] (mllm_hip_fa2) | K rows + the transposed fp16 V slab (mllm_hip_fa2_vt)
CELLS = [(ROWS, D, f16, causal) for D in FA2_D for f16 in (False, True) for causal in (False, True)] + [(VT, D, True, causal) for D in FA2_VT_D for causal in (False, True)]
F16_CELLS = [c for c in CELLS if c[2]]
CAUSAL_CELLS = [c for c in CELLS if c[3]]


def cell_id(cell):
    form, D, f16, causal = cell
    return "%s-D%d-%s-%s" % (form, D, "f16" if f16 else "f32", "causal" if causal else "full")


# ---- (a) Sq = Sk on the row-block and chunk edges; 5 / 33 / 65 end in a partial row tile (nr = 1) that lies on the diagonal when causal; 65 is three row blocks, and its first
#          one is the only causal shape of (a) / (b) whose klim (36) cuts the chunk walk short
SQUARE = [4, 5, FA_R - 1, FA_R, FA_R + 1, 2 * FA_KCH + 1]
# ---- (b) a short query block under the chunk edges (delta > 0)
SHORT_SQ = 8
SHORT_SK = [FA_KCH - 1, FA_KCH, FA_KCH + 1, 2 * FA_KCH - 1, 2 * FA_KCH, 2 * FA_KCH + 1, 3 * FA_KCH + 1]
# ---- the causal cut itself.  klim < sk_eff needs r0 + FA_R + 4 < Sq, i.e. a row block that is not the last: (b)'s eight rows never meet it.  Sq = 40 has the blocks r0 = 0
#      (klim = 36 + delta) and r0 = 32 (no cut); delta = 27, 28, 29 put the first block's cut one key inside chunk 1's end, on the boundary 64, and one key into chunk 2
KLIM_SQ = FA_R + 8
KLIM_SK = [KLIM_SQ + 2 * FA_KCH - FA_R - 4 + e for e in (-1, 0, 1)]
# ---- (c) the fp16 leftover rule on the prefill path: every Sk from 4 to 16; sk_eff < Sk exactly for 5, 6, 7, 10, 11, 15
F16_LEFT_SQ = (4, 6)
F16_LEFT_SK = list(range(4, 17))
F16_LEFT_DROPS = {5: 4, 6: 4, 7: 4, 10: 8, 11: 9, 15: 12}      # Sk: sk_eff
# ---- (d) causal with more queries than keys: the reference's literal reading (rows without a live tile are 0 * (1 / 0) = NaN)
NEG_DELTA = [(8, 7), (12, 8)]
# ---- (e) Br = Bc = 1: one decode launch per row
TINY_SQ = (2, 3)


def tiny_sk(Sq):
    return (Sq, Sq + 5)


# ---- (f) the online-softmax rescale.  LITERAL: test_fa2_online_softmax_rescale_is_forced's construction (Sq = Sk = 96, one head, causal, small keys, key j = 3 q[95]) with the
#      spike in chunk 1 and in tile 0 of chunk 2.  STEPPED: eight rows that see all 96 keys; key 0 is built to hold every row's maximum, so nothing moves until the spiked key,
#      which is built to raise every row's maximum: key 70 = a move in chunk 2 behind a chunk without one; key 64 = tile 0 of a chunk, whose previous maximum is the carried one
RESCALE_LITERAL_SPIKES = (FA_KCH + 9, 2 * FA_KCH)
RESCALE_STEPPED_SPIKES = (2 * FA_KCH + 6, 2 * FA_KCH)
RESCALE_S = 3 * FA_KCH
# ---- heads, once per D and K/V type (Sq = Sk = 65, causal): the (Hq & 7) == 0 remap with three row blocks, without and with a GQA group of 4; no remap with a group of 2; one head
HEADS = [(8, 8), (8, 2), (6, 3), (1, 1)]
HEADS_S = 2 * FA_KCH + 1
# ---- the batch form, once per D and K/V type, causal and not
BATCH_NB, BATCH_SQ, BATCH_SK = 3, FA_R + 1, (FA_R + 1, FA_R + 8)


def sk_eff(Sk, f16):
    tc = Sk // 4
    return 4 * tc + ((Sk % tc if tc else 0) if f16 else Sk % 4)


def klim(r0, Sq, Sk, f16, causal):
    e = sk_eff(Sk, f16)
    return min(e, r0 + FA_R + (Sk - Sq) + 4) if causal else e


def vt_min_ld(Sq, Sk):
    unit = FA_KCH if Sq >= 4 else FA_VCH
    return -(-Sk // unit) * unit


def heads_of(D):
    """(Hq, Hkv) of the cases that are not about heads: a GQA group of 2, heads 2 or 4."""
    return (4, 2) if D <= 64 else (2, 1)


def pitches(Hq, Hkv, D):
    """(ldq, ldk, ldv, ldo) of the engine's kind: Q is the fused q|k|v buffer; K / V rows go on for 8 / 16 more values (16-byte aligned for fp16 and fp32 alike); O has a
    pad of three values (its stores are scalar)."""
    return (Hq + 2 * Hkv) * D, Hkv * D + 8, Hkv * D + 16, Hq * D + 3


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------------------------------------------
def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def qkv(tag, Sq, Sk, Hq, Hkv, D, f16):
    """Seeded standard normals q [Sq][Hq D], k, v [Sk][Hkv D]; K/V of the fp16 instances are rounded to fp16 first (and returned as fp16)."""
    r = np.random.default_rng(seed_of(tag, Sq, Sk, Hq, Hkv, D))
    q = r.standard_normal((Sq, Hq * D)).astype(np.float32)
    k = r.standard_normal((Sk, Hkv * D)).astype(np.float32)
    v = r.standard_normal((Sk, Hkv * D)).astype(np.float32)
    if f16:
        k, v = k.astype(np.float16), v.astype(np.float16)
    return q, k, v


def key_scoring(q, Hq, Hkv, D, level):
    """One key row [Hkv D] whose scaled score q . k / sqrt(D) is `level` for every query row of every head (the rows of a K/V group number at most D, so the least-norm
    solution of the group's linear system exists)."""
    Sq = q.shape[0]
    g = Hq // Hkv
    out = np.empty(Hkv * D, dtype=np.float32)
    for kvh in range(Hkv):
        A = q.reshape(Sq, Hq, D)[:, kvh * g:(kvh + 1) * g, :].reshape(Sq * g, D).astype(np.float64)
        assert A.shape[0] <= D
        out[kvh * D:(kvh + 1) * D] = np.linalg.pinv(A) @ np.full(A.shape[0], level * np.sqrt(D))
    return out


def f16_left_case(Sq, Sk, D):
    """(c): heads_of(D) without a group (Hq = Hkv = 2: at most 6 rows per K/V head); the keys the fp16 rule drops (sk_eff .. Sk - 1) score +40 with every row -- read, they
    would take all the probability -- and their values are large."""
    Hq = Hkv = 2
    q, k, v = qkv("left", Sq, Sk, Hq, Hkv, D, False)
    for j in range(sk_eff(Sk, True), Sk):
        k[j] = key_scoring(q, Hq, Hkv, D, 40.0)
        v[j] = 100.0 + j
    return Hq, Hkv, q, k.astype(np.float16), v.astype(np.float16)


def rescale_literal_case(D, spike):
    S = RESCALE_S
    r = np.random.default_rng(seed_of("rescale", D, spike))
    q = r.standard_normal((S, D)).astype(np.float32)
    k = r.standard_normal((S, D)).astype(np.float32) * 0.1
    v = r.standard_normal((S, D)).astype(np.float32)
    k[spike] = q[S - 1] * 3
    return q, k.astype(np.float16), v.astype(np.float16)


def rescale_stepped_case(D, spike):
    """Sq = 8, Sk = 96, one head, not causal: scaled scores are +6 at key 0, +30 at key `spike`, about 0.1 N(0, 1) elsewhere."""
    r = np.random.default_rng(seed_of("stepped", D, spike))
    q = r.standard_normal((SHORT_SQ, D)).astype(np.float32)
    k = r.standard_normal((RESCALE_S, D)).astype(np.float32) * 0.1
    v = r.standard_normal((RESCALE_S, D)).astype(np.float32)
    k[0] = key_scoring(q, 1, 1, D, 6.0)
    k[spike] = key_scoring(q, 1, 1, D, 30.0)
    return q, k.astype(np.float16), v.astype(np.float16)

"""The Linear kernel instances tests/test_gpu_linear_forms.py launches, as data: which K / super-block counts reach which template instance of
csrc/kernels_linear.hip and csrc/kernels_decode.hip, and the seeded inputs of every case.  Importable without torch or a GPU: tests/test_linear_forms_host.py reads the
launchers' instance lists out of the source and holds this table against them, and checks on the oracle alone that these inputs tell a wrong kernel from a right one.

The instance rules below restate the launchers by hand (they are never asked of the library):
  gemv_q4k_kernel<NSTEPS, ROWS>    launch_gemv_q4k: NSTEPS = ceil(nb / 8), nb = K / 256; one GEMV_CASE(NSTEPS, ROWS) per NSTEPS, anything else is refused
  gemv_q40_kernel<BPL, LPR>        mllm_hip_linear_q40_q80: LPR = 16 when K % 512 == 0 and K / 512 <= 8, else 8; BPL = K / 32 / LPR; one Q40_CASE(BPL, LPR) each
  dec_proj_blk_kernel<8, NS>       dec_linear_row_q4k (mllm_hip_linear, M == 1, fp32 out): NS = ceil(nb / 8) <= 5 and N >= pjb_rows_per_wg, else the two-launch GEMV route
"""
import zlib

import numpy as np

from mllm_amd import lib, synth

# ---- Q4_K GEMV (mllm_hip_linear_q4k_q8k, M < 16) ----------------------------------------------------------------------------------------------------------------------
# nb = K / 256: both ends of every instance's range (8 (NS - 1) + 1 .. 8 NS) and tails that leave lane groups of the last step idle (nb % 8 != 0)
Q4K_GEMV_NB = [1, 7, 8, 9, 16, 17, 23, 24, 25, 32, 33, 35, 40, 41, 47, 48]
Q4K_GEMV_NB_REFUSED = 49          # one past the last instance: MLLM_HIP_ERR_SHAPE before any launch
Q4K_GEMV_M = (1, 2, 15)
Q4K_GEMV_N = 37                   # the last wave's batch of ROWS rows is partial for ROWS = 4, 2 and 1
# rows_per_wave > ROWS (a wave loops over a second batch of rows): N just past 6144 waves x ROWS rows
Q4K_GEMV_SECOND_BATCH = [(1, 24581), (9, 12293), (25, 6150)]        # (nb, N), each at M = 1 and 3
Q4K_GEMV_FEW_ROWS = [(1, 1), (1, 2), (1, 3), (9, 1)]                # (nb, N) with N < ROWS, at M = 2


def q4k_gemv_nsteps(nb):
    return (nb + 7) // 8


# ---- Q4_0 GEMV (mllm_hip_linear_q40_q80) ------------------------------------------------------------------------------------------------------------------------------
Q40_K = [256 * j for j in range(1, 17)]      # all sixteen instances: K an odd multiple of 256 -> 8 lanes per row, a multiple of 512 -> 16
Q40_K_REFUSED = [4352, 4608, 8192]
Q40_M = (1, 2, 15)
Q40_N = 19                                   # ragged against the 8-row pass


def q40_instance(K):
    """(BPL, LPR) of the launcher's choice for rows of K values."""
    lpr = 16 if (K % 512 == 0 and K // 512 <= 8) else 8
    return K // 32 // lpr, lpr


# ---- the one-launch row form (mllm_hip_linear, Q4_K, M == 1, fp32 out -> dec_linear_row_q4k) -------------------------------------------------------------------------------
def pjb_rows_per_wg(nb, N):
    return max(1, min(512 // nb, 32, (N + 255) // 256))


def row_form_ns(nb, N):
    """NS of the dec_proj_blk_kernel<8, NS> instance the generic entry launches for one row, or None where it falls through to quantiser + GEMV."""
    ns = (nb + 7) // 8
    return ns if ns <= 5 and N >= pjb_rows_per_wg(nb, N) else None


# (K, N) of test_linear_q4k_gemv_vs_oracle's M = 1 cases (tests/test_gpu_ops.py), re-run through the generic entry
ROW_FORM_OPS_LIST = [(1536, 2048), (8960, 1536), (256, 64), (1280, 3840), (11008, 128), (1536, 8960), (1536, 8950), (512, 1000), (256, 8229), (2560, 31), (256, 1)]
# (nb, N) at the edges of pjb_rows_per_wg = min(512 / nb, 32, ceil(N / 256)): 1 row (N = 1 is in the list above); 1 -> 2 rows; the cap of 32 with a ragged last workgroup; 512 / 17 = 30 rows;
# 12 rows at the NS = 5 end; both ends of NS = 4 (the lists above do not reach it); nb = 41 falls through to the GEMV
ROW_FORM_EDGES = [(1, 255), (1, 257), (1, 8193), (17, 8000), (40, 3100), (25, 1000), (32, 4100), (41, 64)]
ROW_FORM_CASES = [(K // 256, N) for K, N in ROW_FORM_OPS_LIST] + ROW_FORM_EDGES
assert len(set(ROW_FORM_CASES)) == len(ROW_FORM_CASES)


# ---- seeded inputs: one definition for the GPU tests and for the CPU checks of what these inputs can tell apart ------------------------------------------------------------
def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def weights(wdtype, K, N):
    """Raw blocks of an `[N][K]` weight, every field over its whole range (mllm_amd/synth.py); fp32 weights are seeded normals."""
    r = np.random.default_rng(seed_of("W", wdtype, K, N))
    if wdtype == lib.F32:
        return (r.standard_normal((N, K)) * 0.05).astype(np.float32)
    return synth.quantized_blocks(wdtype, r, N * K, std=0.05, full_range=True)


def acts(tag, M, K, N):
    """Seeded normal activations `[M][K]`, another seed for every (tag, M, K, N)."""
    return np.random.default_rng(seed_of("x", tag, M, K, N)).standard_normal((M, K)).astype(np.float32)


def bias_of(tag, K, N):
    return (np.random.default_rng(seed_of("b", tag, K, N)).standard_normal(N) * 0.1).astype(np.float32)

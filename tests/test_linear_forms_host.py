"""CPU side of tests/test_gpu_linear_forms.py.  (1) Its instance table (tests/linear_forms_table.py) is held against the launchers' source: the GEMV_CASE / Q40_CASE lists of
csrc/kernels_linear.hip and the ROW_CASE list of dec_linear_row_q4k (csrc/kernels_decode.hip) are read out of the text, and the table must launch every instance -- adding
an instance without extending the table fails here, as does dropping an entry from the table.  (2) On the oracle alone: the seeded inputs of the GEMV cases tell a kernel that
skipped or repeated a tail block, or met the weights with the wrong activation row, from a right one.  (3) mllm_hip_linear_workspace_bytes is a contract
(integration/hip/HIPOps.cpp lays the workspace out by hand): restated here and compared.  No GPU."""
import os
import re

import numpy as np
import pytest

from mllm_amd import lib
from oracle import oracle as orc
from tests import linear_forms_table as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mllm_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _cases(text, macro, nargs):
    """Argument tuples of every use of `macro(...)` with integer literals (the #define line itself has names, not literals)."""
    pat = r"\b%s\(\s*%s\s*\)" % (macro, r"\s*,\s*".join([r"(\d+)"] * nargs))
    return [tuple(int(v) for v in m) for m in re.findall(pat, text)]


def test_table_launches_every_q4k_gemv_instance():
    cases = _cases(_src("kernels_linear.hip"), "GEMV_CASE", 2)
    ns_src = sorted(ns for ns, _ in cases)
    assert len(cases) >= 6 and len(set(ns_src)) == len(ns_src), cases
    assert ns_src == list(range(1, len(ns_src) + 1)), cases                      # the table's nb ranges below assume NSTEPS = 1 .. max without a gap
    assert "const int nsteps = (nb + 7) / 8;" in _src("kernels_linear.hip")      # the rule T.q4k_gemv_nsteps restates
    for ns in ns_src:                                                            # both ends of every instance's nb range
        assert 8 * (ns - 1) + 1 in T.Q4K_GEMV_NB and 8 * ns in T.Q4K_GEMV_NB, ns
    assert sorted({T.q4k_gemv_nsteps(nb) for nb in T.Q4K_GEMV_NB}) == ns_src    # and nothing in the table that is not an instance
    assert any(nb % 8 not in (0, 1) for nb in T.Q4K_GEMV_NB)                     # tails that leave lane groups idle
    assert T.Q4K_GEMV_NB_REFUSED == 8 * ns_src[-1] + 1                           # just past the last instance: expected to be refused
    assert 1 in T.Q4K_GEMV_M and 15 in T.Q4K_GEMV_M and any(1 < m < 15 for m in T.Q4K_GEMV_M)
    rows = dict(cases)
    for nb, N in T.Q4K_GEMV_SECOND_BATCH:                                        # rows_per_wave = ceil(N / 6144) rounded up to ROWS exceeds ROWS
        assert -(-N // 6144) > rows[T.q4k_gemv_nsteps(nb)], (nb, N)
    assert {rows[T.q4k_gemv_nsteps(nb)] for nb, _ in T.Q4K_GEMV_SECOND_BATCH} == set(rows.values())
    for nb, N in T.Q4K_GEMV_FEW_ROWS:
        assert N < rows[T.q4k_gemv_nsteps(nb)], (nb, N)
    assert "const int target_waves = 256 * 24;" in _src("kernels_linear.hip")


def test_table_launches_every_q40_gemv_instance():
    text = _src("kernels_linear.hip")
    cases = _cases(text, "Q40_CASE", 2)
    assert len(cases) >= 16 and len(set(cases)) == len(cases), cases
    assert "const int lpr = (K % 512 == 0 && K / 512 <= 8) ? 16 : 8;" in text and "const int bpl = K / 32 / lpr;" in text      # the rule T.q40_instance restates
    reached = [T.q40_instance(K) for K in T.Q40_K]
    assert sorted(reached) == sorted(cases), (sorted(set(cases) - set(reached)), sorted(set(reached) - set(cases)))
    for K in T.Q40_K_REFUSED:
        assert K % 256 == 0 and T.q40_instance(K) not in cases, K
    assert 1 in T.Q40_M and 15 in T.Q40_M and any(1 < m < 15 for m in T.Q40_M)


def test_table_launches_every_one_row_instance():
    text = _src("kernels_decode.hip")
    body = text[text.index("int dec_linear_row_q4k("):]
    body = body[:body.index("#undef ROW_CASE")]
    sw = re.search(r"switch \(nsr\) \{([^}]*)\}", body)
    assert sw, "dec_linear_row_q4k's switch (nsr)"
    ns_src = sorted(n for (n,) in _cases(sw.group(1), "ROW_CASE", 1))
    assert len(ns_src) >= 5
    assert "if (nsr > %d || N < rpw) return 1;" % ns_src[-1] in body             # the fall-through T.row_form_ns restates
    assert "std::max(1, std::min(std::min(512 / (K / 256), 32), (N + 255) / 256))" in text      # pjb_rows_per_wg, restated as T.pjb_rows_per_wg
    reached = {T.row_form_ns(nb, N) for nb, N in T.ROW_FORM_CASES}
    assert None in reached                                                      # a shape that falls through to quantiser + GEMV
    assert sorted(reached - {None}) == ns_src, (sorted(reached - {None}), ns_src)
    # the edges of the rows-per-workgroup rule: one row, the cap of 32 with a ragged last workgroup, a count set by 512 / nb; a lane per super-block and a lane pair
    rpw = {(nb, N): T.pjb_rows_per_wg(nb, N) for nb, N in T.ROW_FORM_CASES if T.row_form_ns(nb, N)}
    assert 1 in rpw.values() and 2 in rpw.values() and any(r == 32 and N % 32 for (nb, N), r in rpw.items())
    assert any(r == 512 // nb and r < 32 and N % r for (nb, N), r in rpw.items())
    assert any(64 < r * nb <= 256 for (nb, N), r in rpw.items()) and any(r * nb > 256 for (nb, N), r in rpw.items())


def _changed(a, b):
    return float(np.mean(a.view(np.uint32) != b.view(np.uint32)))


def _telling(wdtype, tag, K, N, block):
    """At M = 2 on the oracle: zeroing the last `block` activation values, and swapping the two activation rows, each change at least 99 % of the outputs; all are finite."""
    W, x, b = T.weights(wdtype, K, N), T.acts(tag, 2, K, N), T.bias_of(tag, K, N)
    y = orc.linear(x, W, wdtype, N, b)
    assert np.isfinite(y).all(), (K, N)
    xz = x.copy()
    xz[:, K - block:] = 0.0
    assert _changed(orc.linear(xz, W, wdtype, N, b), y) >= 0.99, ("tail block", K, N)
    assert _changed(orc.linear(x[::-1], W, wdtype, N, b), y) >= 0.99, ("rows swapped", K, N)


@pytest.mark.parametrize("nb", T.Q4K_GEMV_NB)
def test_q4k_gemv_inputs_tell_a_wrong_tail_block_or_row(nb):
    _telling(lib.Q4_K, "gemv", 256 * nb, T.Q4K_GEMV_N, 256)


@pytest.mark.parametrize("K", T.Q40_K)
def test_q40_gemv_inputs_tell_a_wrong_tail_block_or_row(K):
    _telling(lib.Q4_0, "q4_0", K, T.Q40_N, 32)


def test_linear_workspace_bytes_is_the_documented_layout():
    so = lib.load()

    def a256(v):
        return (v + 255) & ~255

    for M, K in [(1, 256), (3, 768), (15, 12288), (40, 1280)]:
        want = {lib.Q4_K: a256(M * K) + a256(M * (K // 256) * 4) + a256(M * (K // 16) * 2),      # int8 values | fp32 d per 256 | int16 sums per 16
                lib.Q4_0: a256(M * K) + a256(M * (K // 32) * 2),                                 # int8 values | fp16 d per 32
                lib.F32: 0}
        for dt, w in want.items():
            assert so.mllm_hip_linear_workspace_bytes(dt, M, K) == w, (dt, M, K)

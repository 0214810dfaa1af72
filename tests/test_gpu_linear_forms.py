"""Every Linear kernel instance, row count and output pitch at op level: each template instance of csrc/kernels_linear.hip's GEMVs, the one-launch row form behind the generic
entry (mllm_hip_linear -> dec_linear_row_q4k), the cutovers between kernels and the fp32 dispatch edges, launched through the C ABI at the smallest shapes that reach them.
The instance lists and the seeded inputs live in tests/linear_forms_table.py; tests/test_linear_forms_host.py holds that table against the launchers' source.

Bar: every comparison is against oracle.linear on the same bytes, on the bit patterns (uint32 / uint16 views, so -0.0 and 0.0 differ); weights are drawn over every field's
whole range; wherever the output pitch exceeds N every pad column must still hold the sentinel the harness put there; a refused call leaves the whole output untouched."""
import functools

import numpy as np
import pytest

from tests import linear_forms_table as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mllm_amd import lib, ops  # noqa: E402
from oracle import oracle as orc  # noqa: E402

Q4_K, Q4_0, F32 = lib.Q4_K, lib.Q4_0, lib.F32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    ops.require_gpu()


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def weights(wdtype, K, N):
    return _ro(T.weights(wdtype, K, N))


@functools.lru_cache(maxsize=None)
def acts(tag, M, K, N):
    return _ro(T.acts(tag, M, K, N))


@functools.lru_cache(maxsize=None)
def bias_of(tag, K, N):
    return _ro(T.bias_of(tag, K, N))


@functools.lru_cache(maxsize=None)
def ref_linear(wdtype, tag, M, K, N, f16=False):
    """The oracle on the case's bytes, bias on; computed once and shared (read-only) by the tests that launch the same case through another entry."""
    return _ro(orc.linear(acts(tag, M, K, N), weights(wdtype, K, N), wdtype, N, bias_of(tag, K, N), out_f16=f16))


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return a.view(np.uint16) if a.dtype.itemsize == 2 else a.view(np.uint32)


def assert_bits(y, ref, what):
    """Columns 0 .. N-1 of the device output `[M][ld]` equal `ref [M][N]` bit for bit, and every pad column still holds the sentinel."""
    N = ref.shape[1]
    yb, rb = bits(y), bits(ref)
    assert yb.shape[0] == rb.shape[0] and yb.shape[1] >= N, (what, yb.shape, rb.shape)
    bad = np.argwhere(yb[:, :N] != rb)
    assert bad.size == 0, (what, f"{len(bad)} of {rb.size} differ, first at {bad[0].tolist()}")
    if yb.shape[1] > N:
        assert ops.is_sentinel(y)[:, N:].all(), (what, "pad columns written")


def refused(call, y, what):
    """`call` fails with MLLM_HIP_ERR_SHAPE and `y`, the sentinel-filled output it was given, is untouched.  Returns the error text."""
    with pytest.raises(lib.MllmHipError, match=r"code %d\b" % lib.ERR_SHAPE) as e:
        call()
    torch.cuda.synchronize()
    assert ops.is_sentinel(y).all(), (what, "a refused call wrote to its output")
    return str(e.value)


# ---- Q4_K GEMV: mllm_hip_linear_q4k_q8k, M < 16 (gemv_q4k_kernel<NSTEPS, ROWS>) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", T.Q4K_GEMV_NB)
def test_q4k_gemv_every_instance_and_row_count(nb):
    K, N = 256 * nb, T.Q4K_GEMV_N
    for M in T.Q4K_GEMV_M:
        y = ops.linear_q4k(weights(Q4_K, K, N), acts("gemv", M, K, N), N, bias=bias_of("gemv", K, N))
        assert_bits(y, ref_linear(Q4_K, "gemv", M, K, N), (nb, M))


def test_q4k_gemv_refuses_rows_past_the_last_instance():
    K, N = 256 * T.Q4K_GEMV_NB_REFUSED, T.Q4K_GEMV_N
    for M in (1, 2):
        y = ops.sentinel_out(M, N)
        refused(lambda: ops.linear_q4k(weights(Q4_K, K, N), acts("gemv", M, K, N), N, bias=bias_of("gemv", K, N), out=y), y, (K, M))


@pytest.mark.parametrize("nb,N", T.Q4K_GEMV_SECOND_BATCH)
def test_q4k_gemv_wave_loops_over_a_second_batch_of_rows(nb, N):
    K = 256 * nb
    for M in (1, 3):
        y = ops.linear_q4k(weights(Q4_K, K, N), acts("gemv", M, K, N), N, bias=bias_of("gemv", K, N))
        assert_bits(y, ref_linear(Q4_K, "gemv", M, K, N), (nb, N, M))


def test_q4k_gemv_fewer_rows_than_a_batch():
    for nb, N in T.Q4K_GEMV_FEW_ROWS:
        K, M = 256 * nb, 2
        y = ops.linear_q4k(weights(Q4_K, K, N), acts("gemv", M, K, N), N, bias=bias_of("gemv", K, N), ldy=N + 2)
        assert_bits(y, ref_linear(Q4_K, "gemv", M, K, N), (nb, N))


# M = 1, 5: the GEMV; M = 40, N = 70: the GEMM, whose epilogue is split over a wave pair.  The residual shares the output's pitch.
@pytest.mark.parametrize("M,K,N", [(1, 768, 100), (5, 768, 100), (40, 768, 70)])
def test_q4k_output_pitch(M, K, N):
    W, x, b = weights(Q4_K, K, N), acts("pitch", M, K, N), bias_of("pitch", K, N)
    ref = ref_linear(Q4_K, "pitch", M, K, N)
    assert_bits(ops.linear_q4k(W, x, N, bias=b, ldy=N + 3), ref, "fp32")
    res = np.random.default_rng(T.seed_of("res", M, K, N)).standard_normal((M, N + 3)).astype(np.float32)
    assert_bits(ops.linear_q4k(W, x, N, bias=b, residual=res, ldy=N + 3), ref + res[:, :N], "fp32 + residual")
    assert_bits(ops.linear_q4k(W, x, N, bias=b, out_f16=True, ldy=N + 5), ref_linear(Q4_K, "pitch", M, K, N, f16=True), "fp16")


def test_q4k_cutover_from_gemv_to_gemm():
    """M = 15 is the GEMV's last row count, 16 the GEMM's first: same weights, same first 15 activation rows; each run equals the oracle and rows 0 .. 14 agree across them."""
    K, N = 768, 100
    W, b, x17 = weights(Q4_K, K, N), bias_of("cutover", K, N), acts("cutover", 17, K, N)
    runs = {}
    for M in (15, 16, 17):
        y = ops.linear_q4k(W, x17[:M], N, bias=b)
        assert_bits(y, orc.linear(x17[:M], W, Q4_K, N, b), M)
        runs[M] = bits(y)[:15]
    assert np.array_equal(runs[15], runs[16]) and np.array_equal(runs[15], runs[17])


# ---- the generic entry: mllm_hip_linear (ops.linear); every call must leave the guard band behind its workspace intact ---------------------------------------------------
def generic(wdtype, tag, M, K, N, f16=False, ldy=None):
    y, guard_ok = ops.linear(weights(wdtype, K, N), wdtype, acts(tag, M, K, N), N, bias=bias_of(tag, K, N), out_f16=f16, ldy=ldy)
    assert guard_ok, ("workspace overrun", wdtype, tag, M, K, N)
    assert_bits(y, ref_linear(wdtype, tag, M, K, N, f16=f16), (wdtype, tag, M, K, N, f16, ldy))


@pytest.mark.parametrize("nb,N", T.ROW_FORM_CASES)
def test_generic_q4k_one_row(nb, N):
    """M = 1, fp32 out: the one-launch row form dec_proj_blk_kernel<8, NS> (T.row_form_ns), or quantiser + GEMV where it does not serve the shape."""
    generic(Q4_K, "row", 1, 256 * nb, N)


def test_generic_q4k_other_routes():
    generic(Q4_K, "row", 1, 768, 100, f16=True)             # M = 1 with an fp16 output: quantiser + GEMV
    generic(Q4_K, "row", 1, 768, 100, ldy=103)
    for M in (2, 15):                                        # quantiser + GEMV
        generic(Q4_K, "rows", M, 768, 100)
    for M in (16, 33):                                       # quantiser + the packed GEMM on stream-ordered scratch
        for K, N in ((512, 96), (1280, 70)):
            generic(Q4_K, "rows", M, K, N)
    generic(Q4_K, "rows", 33, 1280, 70, ldy=73)
    generic(Q4_K, "rows", 2, 768, 100, ldy=103)
    generic(Q4_K, "rows", 16, 512, 96, f16=True, ldy=101)


def test_generic_q40_and_f32():
    generic(Q4_0, "g", 1, 256, 7)                            # N K / 2 = 896 is no multiple of 256: the scale plane sits at byte 1024
    generic(Q4_0, "g", 3, 768, 19)
    generic(Q4_0, "g", 3, 768, 19, ldy=22)
    generic(F32, "g", 32, 256, 40)                           # the matrix-core kernel
    generic(F32, "g", 5, 256, 40)                            # the VALU kernel
    generic(F32, "g", 32, 256, 40, ldy=41)


# ---- Q4_0 GEMV: mllm_hip_linear_q40_q80 (gemv_q40_kernel<BPL, LPR>) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", T.Q40_K)
def test_q40_gemv_every_instance_and_row_count(K):
    N = T.Q40_N
    for M in T.Q40_M:
        y = ops.linear_q40(weights(Q4_0, K, N), acts("q4_0", M, K, N), N, bias=bias_of("q4_0", K, N))
        assert_bits(y, ref_linear(Q4_0, "q4_0", M, K, N), (K, T.q40_instance(K), M))


@pytest.mark.parametrize("K", [768, 1024])
def test_q40_rows_split_into_launches_of_fifteen(K):
    N = T.Q40_N
    for M in (16, 30, 31):
        y = ops.linear_q40(weights(Q4_0, K, N), acts("q4_0", M, K, N), N, bias=bias_of("q4_0", K, N), ldy=N + 3)
        assert_bits(y, ref_linear(Q4_0, "q4_0", M, K, N), (K, M))


def test_q40_gemv_few_rows_and_sixteen_rows_per_wave():
    for M, K, N in [(2, 256, 1), (2, 256, 7), (2, 256, 8), (2, 256, 9), (2, 256, 16391)]:
        y = ops.linear_q40(weights(Q4_0, K, N), acts("q4_0", M, K, N), N, bias=bias_of("q4_0", K, N), ldy=N + 1)
        assert_bits(y, ref_linear(Q4_0, "q4_0", M, K, N), (M, K, N))


@pytest.mark.parametrize("K", T.Q40_K_REFUSED)
def test_q40_refuses_rows_without_an_instance(K):
    M, N = 2, T.Q40_N
    y = ops.sentinel_out(M, N)
    msg = refused(lambda: ops.linear_q40(weights(Q4_0, K, N), acts("q4_0", M, K, N), N, bias=bias_of("q4_0", K, N), out=y), y, K)
    assert f"K = {K}" in msg, msg


# ---- fp32 Linear: mllm_hip_linear_f32; the matrix-core kernel when M >= 16, K >= 128, K % 4 == 0 and W, x are 16-byte aligned, else the VALU kernel ---------------------------
def f32_run(M, K, N, **kw):
    return ops.linear_f32(weights(F32, K, N), acts("f32", M, K, N), bias=bias_of("f32", K, N), **kw)


def test_f32_dispatch_edges():
    for M, K, N in [(15, 256, 40), (16, 256, 40), (32, 124, 40), (32, 128, 40), (32, 132, 40)]:
        assert_bits(f32_run(M, K, N), ref_linear(F32, "f32", M, K, N), (M, K, N))


def test_f32_operands_off_a_sixteen_byte_boundary():
    M, K, N = 32, 256, 40
    ref = ref_linear(F32, "f32", M, K, N)
    aligned = f32_run(M, K, N)
    assert_bits(aligned, ref, "aligned")
    for w_off, x_off in ((True, False), (False, True), (True, True)):
        y = f32_run(M, K, N, w_off=w_off, x_off=x_off)
        assert_bits(y, ref, (w_off, x_off))
        assert np.array_equal(bits(y), bits(aligned)), (w_off, x_off)


def test_f32_output_pitch():
    for M, K, N in [(32, 256, 33), (5, 256, 33)]:             # the matrix-core kernel, the VALU kernel
        assert_bits(f32_run(M, K, N, ldy=N + 1), ref_linear(F32, "f32", M, K, N), (M, K, N))

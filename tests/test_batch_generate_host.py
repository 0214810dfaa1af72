"""Host side of the device-resident batched generation (mllm_hip_model_batch_generate): the entry point exists and refuses a NULL model without touching HIP, and the
rotary table the batched step keeps resident is, row for row and bit for bit, what the per-step host call produced for that position."""
import ctypes as C

import numpy as np

from mllm_amd import synth


def test_batch_generate_is_declared_exported_and_refuses_a_null_model():
    from mllm_amd import lib
    assert "mllm_hip_model_batch_generate" in lib.declared_symbols()
    assert "mllm_hip_mrope_decode_table" in lib.declared_symbols()
    L = lib.load()
    fn = L.mllm_hip_model_batch_generate          # AttributeError when the library does not export it
    first = (C.c_int32 * 2)(1, 2)
    rc = fn(C.c_void_p(0), C.c_int(2), first, C.c_int(4), C.c_int32(-1), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0))
    assert rc == lib.ERR_ARG


def test_mrope_decode_table_rows_equal_the_per_step_rows():
    """In decode all three M-RoPE axes hold one position (modeling_qwen2_vl.hpp:423-432), so a step's rotary row is a function of that integer alone.  The table the batched
    step indexes on the device is built once for positions 0 .. cache_limit - 1; every row equals the row mllm_hip_mrope_table gives when called for that single position,
    which is what mllm_hip_model_batch_decode computed on the host per step."""
    from mllm_amd import lib
    cfg = synth.qwen2vl_tiny()
    D = cfg.hidden // cfg.heads
    s_tab, c_tab = lib.mrope_decode_table(cfg.rope_theta, D, cfg.cache_limit, cfg.mrope_section)
    assert s_tab.shape == (cfg.cache_limit, D // 2)
    for p in range(cfg.cache_limit):
        s1, c1 = lib.mrope_table(cfg.rope_theta, D, np.full((3, 1), float(p), dtype=np.float32), cfg.mrope_section)
        assert np.array_equal(s_tab[p], s1[0]) and np.array_equal(c_tab[p], c1[0]), p
    # and for a batch of sequences at different positions in one call, as the per-step form gathered them
    pos = np.asarray([[5, 40, 23, 95]] * 3, dtype=np.float32)
    s4, c4 = lib.mrope_table(cfg.rope_theta, D, pos, cfg.mrope_section)
    assert np.array_equal(s4, s_tab[[5, 40, 23, 95]]) and np.array_equal(c4, c_tab[[5, 40, 23, 95]])
    assert len(np.unique(s_tab, axis=0)) == cfg.cache_limit          # the rows differ: an index slip cannot pass

"""Batched prefill (mllm_hip_model_batch_prefill), the parts that need no GPU: the header declares the entry point, the built library exports it and refuses a NULL model,
and lib.Model.batch_prefill has the documented signature.  The arithmetic contract is tests/test_batch_prefill.py (MI355X)."""
import ctypes as C
import inspect


def test_batch_prefill_is_declared_exported_and_refuses_a_null_model():
    from mllm_amd import lib
    assert "mllm_hip_model_batch_prefill" in lib.declared_symbols()
    fn = lib.load().mllm_hip_model_batch_prefill          # AttributeError when the library does not export it
    ids = (C.c_int32 * 3)(1, 2, 3)
    n = (C.c_int32 * 2)(2, 1)
    rc = fn(C.c_void_p(0), C.c_int(2), ids, n, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0))
    assert rc == lib.ERR_ARG


def test_model_batch_prefill_signature():
    from mllm_amd import lib
    sig = inspect.signature(lib.Model.batch_prefill)
    assert list(sig.parameters) == ["self", "prompts", "visual_dev", "grid_thw", "n_visual_rows", "want_logits"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["visual_dev"] is None and d["grid_thw"] is None and d["n_visual_rows"] is None and d["want_logits"] is True

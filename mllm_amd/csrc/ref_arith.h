// mllm_amd/csrc/ref_arith.h -- the reference's arithmetic rules, each written once (bit-equality with the reference's evaluation order).
// Leaf functions only: one rule, one function.  Who sums what in which order, the lane mapping, the loads and the stores stay with the kernels.
// Included at the end of common.h (the wave helpers above it are what the Q8_K and first-maximum steps are built from).
#pragma once

namespace mllm_hip {

// ---- A14: the reference's AVX2 polynomial expf, one fp32 lane of it (compute/ActivationFunction.hpp:96-134 mllm_v_expf): same constants, same fma placement ----
__device__ __forceinline__ float ref_expf_poly(float x) {
    const float r = 0x1.8p23f;
    const float z = __fmaf_rn(x, 0x1.715476p+0f, r);
    const float n = __fsub_rn(z, r);
    const float b = __fmaf_rn(-n, 0x1.7f7d1cp-20f, __fmaf_rn(-n, 0x1.62e4p-1f, x));
    const uint32_t e = __float_as_uint(z) << 23;
    const float k = __uint_as_float(e + __float_as_uint(1.0f));
    const bool c = fabsf(n) > 126.0f;
    const float u = __fmul_rn(b, b);
    const float j = __fmaf_rn(__fmaf_rn(__fmaf_rn(0x1.0e4020p-7f, b, 0x1.573e2ep-5f), u, __fmaf_rn(0x1.555e66p-3f, b, 0x1.fffdb6p-2f)), u,
                              __fmul_rn(0x1.ffffecp-1f, b));
    if (!c) return __fmaf_rn(j, k, k);
    const uint32_t g = (n <= 0.0f) ? 0x82000000u : 0u;
    const float s1 = __uint_as_float(g + 0x7f000000u);
    const float s2 = __uint_as_float(e - g);
    if (fabsf(n) > 192.0f) return __fmul_rn(s1, s1);
    return __fmul_rn(__fmaf_rn(s2, j, s2), s1);
}
// x / (1 + exp(-x)) on that polynomial (compute/ActivationFunction.hpp:137-146 mllm_v_silu)
__device__ __forceinline__ float ref_silu(float x) { return __fdiv_rn(x, __fadd_rn(1.0f, ref_expf_poly(__fsub_rn(0.0f, x)))); }

// ---- A4, Q8_0: quantize_row_q8_0 as the reference's x86 build runs it, the AVX2 path (ggml QuantizeQ8.cpp:113-167), not quantize_row_q8_0_reference:
// d = amax/127 (stored fp16), q = rint(x * (127/amax)) -- _mm256_round_ps(_MM_ROUND_NEAREST) takes halves to even.  amax = max |x| of the 32-block. ----
__device__ __forceinline__ void q80_scale(float amax, float &d, float &id) {
    d = __fdiv_rn(amax, 127.0f);
    id = amax != 0.0f ? __fdiv_rn(127.0f, amax) : 0.0f;
}
__device__ __forceinline__ uint32_t q80_round4(const float4 &v, float id) {      // four consecutive values -> their four bytes
    const int q0 = (int)rintf(__fmul_rn(v.x, id)), q1 = (int)rintf(__fmul_rn(v.y, id));
    const int q2 = (int)rintf(__fmul_rn(v.z, id)), q3 = (int)rintf(__fmul_rn(v.w, id));
    return (uint32_t)(q0 & 0xff) | ((uint32_t)(q1 & 0xff) << 8) | ((uint32_t)(q2 & 0xff) << 16) | ((uint32_t)(q3 & 0xff) << 24);
}

// ---- A10/A11/A19: the rope_hf rotary pair (CPUMultimodalRoPE.cpp:153-221).  The reference is built with GCC -O2 -mfma, whose default contraction turns
// `a*c - b*s` into fma(a, c, -(b*s)) and `a*s + b*c` into fma(a, s, b*c). ----
__device__ __forceinline__ void rope_pair(float a, float b, float sn, float cs, float &v1, float &v2) {
    v1 = __fmaf_rn(a, cs, -__fmul_rn(b, sn));
    v2 = __fmaf_rn(a, sn, __fmul_rn(b, cs));
}

// ---- first maximum (std::max_element semantics, processing_qwen2_vl.hpp:284-289): the larger value; among equal values the smaller index ----
// (the merge keeps its `if`: written as a predicate that returns bool, the compiler turns the short-circuit into selects and every caller's instruction sequence changes)
__device__ __forceinline__ void first_max_merge(float &best, int &besti, float v, int i) {
    if (v > best || (v == best && i < besti)) { best = v; besti = i; }
}
__device__ __forceinline__ void wave_first_max(float &best, int &besti) {      // every lane ends with the wave's (value, index)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(besti, m, 64);
        first_max_merge(best, besti, ov, oi);
    }
}
// wave 0's (best, besti) folded with the LDS slots that waves 1 .. NW-1 left
template <int NW>
__device__ __forceinline__ void fold_first_max(const float *sv, const int *si, float &best, int &besti) {
    for (int w = 1; w < NW; ++w) first_max_merge(best, besti, sv[w], si[w]);
}

// ---- N2: the temperature softmax over the candidates of the sampling methods (Generate.cpp:69-87 / :120-136; mllm_hip_topk_probs_host is the host form): every
// step is a double operation on a float promoted to double, rounded once.  The two sums between the steps are sequential and stay with the kernel. ----
__device__ __forceinline__ double cand_exp_arg(float v, double max_logit, float temperature) { return __ddiv_rn(__dsub_rn((double)v, max_logit), (double)temperature); }
__device__ __forceinline__ float cand_over_sum(float e, double sum_exp) { return (float)__ddiv_rn((double)e, sum_exp); }      // probs[i] /= sum_exp (a double)
__device__ __forceinline__ float cand_renorm(float p, float fsum) { return __fdiv_rn(p, fsum); }                              // probs[i] /= _sum (a float)
// The reference rounds exp()'s double to float.  Its libm exp and the device library's are both within 1 ulp of the true value, so they are within 2 double ulps of each
// other: unless the device's double lies that close to a float rounding tie, both round to the same float.  true = this value could round either way.
__device__ __forceinline__ bool f32_rounding_ambiguous(double d) {
    const uint64_t bits = (uint64_t)__double_as_longlong(d);
    const int be = (int)((bits >> 52) & 0x7ff);
    if (be == 0 || be == 0x7ff) return false;      // zero (a double subnormal is a float zero for every neighbour too), infinity, NaN
    const int e = be - 1023;
    const int drop = e >= -126 ? 29 : 29 + (-126 - e);      // significand bits the float does not keep (more of them below the float's normal range)
    if (drop > 54) return false;                              // below 2^-151: zero, whatever the last bits are
    const uint64_t sig = (bits & 0xfffffffffffffull) | (1ull << 52);
    const uint64_t low = sig & ((1ull << drop) - 1), half = 1ull << (drop - 1);
    return (low > half ? low - half : half - low) <= 2;
}
// ---- the inverse-CDF step of the draw (mllm_hip_sample_index_host): acc += probs[i] / sum, both double.  The quotients are independent of each other, so a kernel
// computes them a lane each (cdf_term) and only adds in sequence (cdf_add) ----
__device__ __forceinline__ double cdf_term(float p, double sum) { return __ddiv_rn((double)p, sum); }
__device__ __forceinline__ double cdf_add(double acc, double term) { return __dadd_rn(acc, term); }

// ---- A9 RMSNorm after the sum of squares (op/CPURMSNorm.cpp:31-136): the sum is a double, its mean is rounded to fp32 before eps is added ----
__device__ __forceinline__ float rms_inv(double ss, int dim, float eps) {
    const float m = (float)(ss / (double)dim);
    return __fdiv_rn(1.0f, sqrtf(__fadd_rn(m, eps)));
}
__device__ __forceinline__ float rms_scale(float x, float inv, float w) { return __fmul_rn(__fmul_rn(x, inv), w); }

// ---- A8: dequantize_row_q4_0 (ggml QuantizeQ4.cpp:74-93) of one nibble: y = (nib - 8) * d ----
__device__ __forceinline__ float q40_value(int nibble, float d) { return __fmul_rn((float)(nibble - 8), d); }

// ---- A4, Q8_K: quantize_row_q8_K_reference (ggml QuantizeQ8.cpp:216-251): max = x[first j with largest |x|]; iscale = -128/max; q = min(127, nearest_int(iscale*x));
// d = 1/iscale.  One 256-block is held as 4 consecutive values per lane of one wave. ----
// nearest_int of ggml (Quantize.hpp:174-180): magic-add, round-to-nearest-even. Explicit _rn ops: no contraction.
__device__ __forceinline__ int nearest_int(float v) {
    float val = __fadd_rn(v, 12582912.0f);
    return (__float_as_int(val) & 0x007fffff) - 0x00400000;
}
// The signed first maximum -- the value ggml's strict `>` scan keeps: x[first j with |x[j]| == amax] -- in the steps that a kernel quantising several blocks interleaves
// across them.  The first lane holding +amax or -amax decides the sign; only a lane that holds both (amax != 0) needs the order of its four elements.
// step 1: the lane's largest and smallest value.  v_max3 / v_min3 spelled out: fmaxf() on loaded values is preceded by a canonicalising v_max x, x per operand (IEEE mode)
__device__ __forceinline__ void q8k_hi_lo(const float4 &v, float &hi, float &lo) {
    float t;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(t) : "v"(v.x), "v"(v.y), "v"(v.z));
    asm("v_max_f32 %0, %1, %2" : "=v"(hi) : "v"(t), "v"(v.w));
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(t) : "v"(v.x), "v"(v.y), "v"(v.z));
    asm("v_min_f32 %0, %1, %2" : "=v"(lo) : "v"(t), "v"(v.w));
}
// step 2: bits of amax = max |x| over the block (wave-uniform, >= +0), reduced on the value bits with integer max
__device__ __forceinline__ unsigned q8k_amax_bits(float hi, float lo) {
    float am;
    asm("v_max_f32 %0, |%1|, |%2|" : "=v"(am) : "v"(hi), "v"(lo));
    return wave_umax(__float_as_uint(am));
}
// step 3: bits of the signed maximum from the ballots of the lanes holding +amax / -amax; true when the deciding lane holds both, and step 4 has to decide instead
__device__ __forceinline__ bool q8k_sign(float hi, float lo, unsigned abits, unsigned &mbits) {
    const float amax = __uint_as_float(abits);
    const unsigned long long pos = __ballot(hi == amax), neg = __ballot(lo == -amax);
    const unsigned long long both = pos | neg, first = both & (0ull - both);
    mbits = abits ^ ((neg & first) ? 0x80000000u : 0u);
    return (pos & neg & first) != 0 && abits != 0;
}
// step 4 (the tangled lane; on its own it is also the whole rule): the first element in element order, of the first lane, that attains amax
__device__ __forceinline__ float q8k_first_in_order(const float4 &v, float amax) {
    const float a0 = fabsf(v.x), a1 = fabsf(v.y), a2 = fabsf(v.z), a3 = fabsf(v.w);
    const float mine = a0 == amax ? v.x : (a1 == amax ? v.y : (a2 == amax ? v.z : v.w));
    return first_flagged(a0 == amax || a1 == amax || a2 == amax || a3 == amax, mine);
}
// the four steps for one block; the step 4 case sits behind a wave-uniform branch
__device__ __forceinline__ float q8k_first_max(const float4 &v, unsigned &abits) {
    float hi, lo;
    q8k_hi_lo(v, hi, lo);
    abits = q8k_amax_bits(hi, lo);
    unsigned mbits;
    if (q8k_sign(hi, lo, abits, mbits)) mbits = __float_as_uint(q8k_first_in_order(v, __uint_as_float(abits)));
    return __uint_as_float(mbits);
}
// min(127, nearest_int(iscale * x)) of the lane's four values, left as the BITS of 12582912 + q (the low byte is q's byte; q as a float is bits - 12582912.0f exactly).
// Identical to the reference for every finite product: the clamp to 127 is an unsigned min on the bits.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void q8k_round4(const float4 &v, float iscale, uint32_t (&b)[4]) {
    const f32x2_t s = {iscale, iscale}, magic = {12582912.0f, 12582912.0f};
    const f32x2_t m01 = f32x2_t{v.x, v.y} * s + magic, m23 = f32x2_t{v.z, v.w} * s + magic;      // -ffp-contract=off: a product, then a sum (v_pk_mul_f32, v_pk_add_f32)
    const uint32_t top = 0x4B40007Fu;      // bits of 12582912 + 127
    b[0] = min(__float_as_uint(m01.x), top); b[1] = min(__float_as_uint(m01.y), top);
    b[2] = min(__float_as_uint(m23.x), top); b[3] = min(__float_as_uint(m23.y), top);
}
__device__ __forceinline__ uint32_t q8k_bytes(const uint32_t (&b)[4]) {      // the four q bytes: two v_perm + or
    return __builtin_amdgcn_perm(b[1], b[0], 0x0c0c0400u) | __builtin_amdgcn_perm(b[3], b[2], 0x04000c0cu);
}
__device__ __forceinline__ int q8k_sum4(uint32_t bytes) { return __builtin_amdgcn_sdot4((int)bytes, 0x01010101, 0, false); }      // q0+q1+q2+q3: one v_dot4
__device__ __forceinline__ void q8k_floats(const uint32_t (&b)[4], f32x2_t &q01, f32x2_t &q23) {      // q as floats, exactly
    const f32x2_t unmagic = {-12582912.0f, -12582912.0f};
    q01 = f32x2_t{__uint_as_float(b[0]), __uint_as_float(b[1])} + unmagic;
    q23 = f32x2_t{__uint_as_float(b[2]), __uint_as_float(b[3])} + unmagic;
}

}  // namespace mllm_hip

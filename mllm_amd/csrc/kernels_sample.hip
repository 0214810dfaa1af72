// mllm_amd/csrc/kernels_sample.hip -- SURVEY N2: candidate selection of the sampled generation methods on the device, and the visual-token
// exchange of the sharded vision prefill (RCCL) behind the C ABI.
//
//   _LlmTextGenerateToppSamplingMethod::generate (mllm/Generate.cpp:93-142) sorts the whole (probability, index) row descending (std::sort :99) and keeps
//   the prefix whose running sum reaches p: here the sort is one device radix sort (keys descending; the sort is stable and the indices start ascending, so
//   equal probabilities keep ascending index order -- std::sort leaves ties unspecified), and only the prefix crosses PCIe.
//   The draw of both sampling methods, _sample_element (Generate.hpp:38-44), is a std::discrete_distribution over the float probabilities: the host helper
//   below is its inverse-CDF form on a caller-supplied uniform number (the reference seeds from std::random_device and cannot be replayed).
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>

#include "common.h"
#include "decode_launch.h"

using namespace mllm_hip;

namespace {
__global__ void iota_kernel(int *p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
size_t sort_temp_bytes(int n) {
    size_t tb = 0;
    (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tb, (const float *)nullptr, (float *)nullptr, (const int *)nullptr, (int *)nullptr, n);
    return tb;
}
}  // namespace

extern "C" size_t mllm_hip_sort_desc_workspace_bytes(int n) { return n <= 0 ? 0 : align256((size_t)n * 4) + align256(sort_temp_bytes(n)); }

extern "C" int mllm_hip_sort_desc(const float *x, int n, float *val_sorted, int *idx_sorted, void *workspace, size_t workspace_bytes, void *stream) {
    if (n <= 0 || !x || !val_sorted || !idx_sorted) return MLLM_HIP_ERR_ARG;
    if (!workspace || workspace_bytes < mllm_hip_sort_desc_workspace_bytes(n)) return MLLM_HIP_ERR_ARG;
    hipStream_t st = as_stream(stream);
    int *iota = (int *)workspace;
    void *temp = (uint8_t *)workspace + align256((size_t)n * 4);
    size_t tb = workspace_bytes - align256((size_t)n * 4);
    hipLaunchKernelGGL(iota_kernel, dim3((n + 255) / 256), dim3(256), 0, st, iota, n);
    int rc = MH_LAUNCH_OK("iota");
    if (rc) return rc;
    MH_CHECK(hipcub::DeviceRadixSort::SortPairsDescending(temp, tb, x, val_sorted, (const int *)iota, idx_sorted, n, 0, 32, st));
    return MLLM_HIP_OK;
}

extern "C" int mllm_hip_sample_index_host(const float *probs, int k, float u01) {
    if (!probs || k <= 0) return 0;
    double sum = 0.0;
    for (int i = 0; i < k; ++i) sum += probs[i];
    double acc = 0.0;
    for (int i = 0; i < k; ++i) {
        acc += probs[i] / sum;
        if ((double)u01 < acc) return i;
    }
    return k - 1;
}

// ---- the sampled tail of a batched step ---------------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int TAIL_NT = 256, TAIL_J = 8;      // threads of the tail's workgroup; consecutive values a lane of wave 0 holds per pass of a sequential walk
// The sequential walks below run on wave 0 with a TRAVELLING accumulator (softmax_row_sum_kernel's walk): a pass loads 64 x TAIL_J consecutive values at once, lane l
// holding values l * TAIL_J ..; the accumulator enters lane 0 from lane 63 (wave_ror:1), takes lane 0's values in index order, hops to lane 1, and so on, so after 64
// hops lane 63 holds the pass's result.  The order is the host loop's; an add waits for the add before it and for nothing else.  (The other lanes carry accumulators
// nobody reads.)  A slot behind the end holds +0.0, which changes no sum that started at +0.0.
constexpr int DPP_WAVE_ROR1 = 0x13C;
__device__ __forceinline__ int hop(int v) { return MH_DPP(0, v, DPP_WAVE_ROR1, 0xF); }
__device__ __forceinline__ float hop(float v) { return __int_as_float(hop(__float_as_int(v))); }
__device__ __forceinline__ double hop(double v) { return __hiloint2double(hop(__double2hiint(v)), hop(__double2loint(v))); }
__device__ __forceinline__ int last_lane(int v) { return __builtin_amdgcn_readlane(v, 63); }
__device__ __forceinline__ float last_lane(float v) { return __int_as_float(last_lane(__float_as_int(v))); }
__device__ __forceinline__ double last_lane(double v) { return __hiloint2double(last_lane(__double2hiint(v)), last_lane(__double2loint(v))); }
// double sum of p[0 .. n), in index order, from +0.0
__device__ double serial_dsum(const float *__restrict__ p, int n) {
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int base = 0; base < n; base += 64 * TAIL_J) {
        double u[TAIL_J];
#pragma unroll
        for (int j = 0; j < TAIL_J; ++j) { const int i = base + lane * TAIL_J + j; u[j] = i < n ? (double)p[i] : 0.0; }
        for (int h = 0; h < 64; ++h) {
            s = hop(s);
#pragma unroll
            for (int j = 0; j < TAIL_J; ++j) s = __dadd_rn(s, u[j]);
        }
        s = last_lane(s);
    }
    return s;
}
// `while (p < top_p) p += val[n++]` of Generate.cpp:108-115 in float, bounded by the row: the candidates kept
__device__ int serial_nucleus(const float *__restrict__ val, int n, float top_p) {
    const int lane = threadIdx.x & 63;
    float p = 0.0f;
    int cnt = 0;
    for (int base = 0; base < n && p < top_p; base += 64 * TAIL_J) {
        float u[TAIL_J];
#pragma unroll
        for (int j = 0; j < TAIL_J; ++j) { const int i = base + lane * TAIL_J + j; u[j] = i < n ? val[i] : 0.0f; }
        for (int h = 0; h < 64; ++h) {
            p = hop(p); cnt = hop(cnt);
#pragma unroll
            for (int j = 0; j < TAIL_J; ++j) {
                const bool go = p < top_p && base + lane * TAIL_J + j < n;      // once false it stays false: p no longer changes
                p = go ? __fadd_rn(p, u[j]) : p;
                cnt += go ? 1 : 0;
            }
        }
        p = last_lane(p); cnt = last_lane(cnt);
    }
    return cnt;
}
// mllm_hip_sample_index_host after its sum: the first i with u < acc, else the last candidate
__device__ int serial_cdf_pick(const float *__restrict__ prob, int n, double sum, float u01) {
    const int lane = threadIdx.x & 63;
    const double u = (double)u01;
    double acc = 0.0;
    int pick = -1;
    for (int base = 0; base < n && pick < 0; base += 64 * TAIL_J) {
        double q[TAIL_J];
#pragma unroll
        for (int j = 0; j < TAIL_J; ++j) { const int i = base + lane * TAIL_J + j; q[j] = i < n ? cdf_term(prob[i], sum) : 0.0; }
        for (int h = 0; h < 64; ++h) {
            acc = hop(acc); pick = hop(pick);
#pragma unroll
            for (int j = 0; j < TAIL_J; ++j) {
                const int i = base + lane * TAIL_J + j;
                acc = cdf_add(acc, q[j]);
                pick = (pick < 0 && i < n && u < acc) ? i : pick;
            }
        }
        acc = last_lane(acc); pick = last_lane(pick);
    }
    return pick < 0 ? n - 1 : pick;
}
struct TailArgs {
    const float *val; const int *idx; int64_t ldc;      // row r's candidates, best first, at r * ldc: the k best (top-k) or the whole sorted row (top-p)
    int n_cand, nucleus;                               // candidates there; nucleus != 0: only the prefix that reaches top_p is kept
    float top_p, temperature; const SampleCtl *ctl;    // ctl != nullptr: top_p, temperature and u_ld come from device memory
    const float *u01; const SeqKV *seqs; int cap;
    float *prob;                                       // [rows][ldc]
    int *ids_out, *cand_idx; float *cand_prob; int64_t cand_ld; int *cand_n, *n_ambiguous;
};
// One workgroup per row: nucleus walk (top-p), the candidate softmax of mllm_hip_topk_probs_host bit for bit, the draw of mllm_hip_sample_index_host.  The exp()s and
// the divisions are spread over the workgroup; the three sums and the two walks are wave 0's, in index order.
__global__ __launch_bounds__(TAIL_NT) void sample_tail_kernel(const TailArgs a) {
    __shared__ int s_cnt;
    __shared__ double s_sum;
    __shared__ float s_fsum;
    const int row = blockIdx.x, tid = threadIdx.x;
    float top_p = a.top_p, temperature = a.temperature, u01;
    int u_ld = 1;
    if (a.ctl) { top_p = a.ctl->top_p; temperature = a.ctl->temperature; u_ld = a.ctl->u_ld; }
    if (a.seqs) {
        if (!a.seqs[row].active || a.seqs[row].t >= a.cap) return;      // a stopped row, or one whose cache is full, draws nothing (workgroup-uniform)
        const int made = a.seqs[row].made;
        u01 = made < u_ld ? a.u01[(int64_t)row * u_ld + made] : 0.0f;
    } else {
        u01 = a.u01[row];
    }
    const float *val = a.val + (int64_t)row * a.ldc;
    const int *idx = a.idx + (int64_t)row * a.ldc;
    float *prob = a.prob + (int64_t)row * a.ldc;
    int cnt = a.n_cand;
    if (a.nucleus) {
        if (tid < 64) { const int c = serial_nucleus(val, a.n_cand, top_p); if (tid == 0) s_cnt = c; }
        __syncthreads();
        cnt = s_cnt;
    }
    // the candidates are in descending order: their first maximum (std::max_element) is candidate 0
    const double max_logit = (double)val[0];
    int amb = 0;
    for (int i = tid; i < cnt; i += TAIL_NT) {
        const double e = exp(cand_exp_arg(val[i], max_logit, temperature));
        amb += f32_rounding_ambiguous(e) ? 1 : 0;
        prob[i] = (float)e;
    }
    if (amb && a.n_ambiguous) atomicAdd(a.n_ambiguous, amb);
    __syncthreads();
    if (tid < 64) { const double s = serial_dsum(prob, cnt); if (tid == 0) s_sum = s; }
    __syncthreads();
    const double sum_exp = s_sum;
    for (int i = tid; i < cnt; i += TAIL_NT) prob[i] = cand_over_sum(prob[i], sum_exp);
    __syncthreads();
    if (tid < 64) { const double s = serial_dsum(prob, cnt); if (tid == 0) s_fsum = (float)s; }      // float _sum = std::accumulate(..., 0.0)
    __syncthreads();
    const float fsum = s_fsum;
    for (int i = tid; i < cnt; i += TAIL_NT) {
        const float p = cand_renorm(prob[i], fsum);
        prob[i] = p;
        if (a.cand_prob) a.cand_prob[(int64_t)row * a.cand_ld + i] = p;
        if (a.cand_idx) a.cand_idx[(int64_t)row * a.cand_ld + i] = idx[i];
    }
    __syncthreads();
    if (tid < 64) {
        const double sum = serial_dsum(prob, cnt);
        const int pick = serial_cdf_pick(prob, cnt, sum, u01);
        if (tid == 0) {
            a.ids_out[row] = idx[pick];
            if (a.cand_n) a.cand_n[row] = cnt;
        }
    }
}
// lane b: sequence b.  seqs_next_kernel's advance (kernels_elem.hip) on the drawn id
__global__ __launch_bounds__(64) void seqs_sample_next_kernel(SeqKV *__restrict__ seqs, BatchCtl *__restrict__ ctl, const int *__restrict__ drawn, int B, int cap,
                                                              int *__restrict__ tok_out, float *__restrict__ ids_f, int *__restrict__ history, int hist_ld) {
    const int b = threadIdx.x;
    int on = 0;
    if (b < B) {
        on = seqs[b].active;
        if (on && seqs[b].t < cap) {
            const int made = seqs[b].made, id = drawn[b];
            tok_out[b] = id;
            if (made < hist_ld) history[(int64_t)b * hist_ld + made] = id;
            ids_f[b] = (float)id;      // the embedding reads fp32 ids (ids below 2^24 are exact)
            if (id == ctl->eos) on = 0;      // eos < 0 matches no id
            seqs[b].t += 1;
            seqs[b].pos += 1;
            seqs[b].made = made + 1;
            seqs[b].active = on;
        }
    }
    const int n = __popcll(__ballot(on != 0));
    if (b == 0) ctl->n_active = n;
}
struct SampleWs { float *val; int *idx; float *prob, *soft, *scr; void *sort; size_t sort_bytes, total; int64_t ldc; };
// the workspace's parts: top-k keeps 64 slots per row, top-p whole rows (the nucleus may be the whole row) plus the softmax's and the sort's scratch
SampleWs sample_ws(void *base, int rows, int n, int method, int top_k) {
    SampleWs w{};
    size_t off = 0;
    auto take = [&](size_t bytes) { void *p = base ? (uint8_t *)base + off : nullptr; off += align256(bytes); return p; };
    if (method == 2) {
        w.ldc = n;
        w.soft = (float *)take((size_t)rows * n * 4);
        w.scr = (float *)take(n >= 16384 ? softmax_long_rows_scratch_bytes(rows, n) : 0);
        w.sort_bytes = mllm_hip_sort_desc_workspace_bytes(n);
        w.sort = take(w.sort_bytes);
    } else {
        w.ldc = 64;
        w.scr = (float *)take(rows_topk_scratch_bytes(rows, n, std::max(1, top_k)));
    }
    w.val = (float *)take((size_t)rows * w.ldc * 4);
    w.idx = (int *)take((size_t)rows * w.ldc * 4);
    w.prob = (float *)take((size_t)rows * w.ldc * 4);
    w.total = off;
    return w;
}
}  // namespace

namespace mllm_hip {
size_t sample_rows_workspace_bytes(int rows, int n, int method, int top_k) {
    if (rows <= 0 || n <= 0 || method < 1 || method > 2) return 0;
    return sample_ws(nullptr, rows, n, method, top_k).total;
}
int sample_rows_launch(const SampleRows &a, hipStream_t st) {
    if (!a.x || !a.u01 || !a.ids_out || a.rows <= 0 || a.n <= 0 || a.ld < a.n || a.method < 1 || a.method > 2) return MLLM_HIP_ERR_ARG;
    if ((a.cand_idx || a.cand_prob) && a.cand_ld < (a.method == 2 ? a.n : std::max(1, a.top_k))) return MLLM_HIP_ERR_ARG;
    if (a.method == 1 && (a.top_k < 0 || a.top_k > 64 || a.top_k > a.n)) return MLLM_HIP_ERR_SHAPE;
    if (!a.ctl && (!(a.temperature > 0.0f) || (a.method == 2 && !(a.top_p > 0.0f)))) return MLLM_HIP_ERR_ARG;
    if (!a.ws || a.ws_bytes < sample_rows_workspace_bytes(a.rows, a.n, a.method, a.top_k)) return MLLM_HIP_ERR_ARG;
    const SampleWs w = sample_ws(a.ws, a.rows, a.n, a.method, a.top_k);
    TailArgs t{};
    if (a.method == 1) {
        // k = 0 or 1 is the first-maximum argmax (Generate.cpp:50-54): the one best candidate, which the tail then returns whatever u01 is
        const int k = std::max(1, a.top_k);
        if (int rc = rows_topk_launch(a.x, a.ld, a.rows, a.n, k, w.val, w.idx, (int)w.ldc, w.scr, st)) return rc;
        t.n_cand = k; t.nucleus = 0;
    } else {
        const float *src = a.x;
        int64_t lds = a.ld;
        if (a.softmax_first) {
            // the vocabulary softmax the caller's graph ends in (CPUSoftMax), in mllm_hip_softmax's two forms: one wave per short row, the chip per long row
            if (a.n >= 16384) { if (int rc = softmax_long_rows_launch(a.x, a.ld, w.soft, a.n, a.rows, a.n, w.scr, st)) return rc; }
            else if (a.ld == a.n) { if (int rc = mllm_hip_softmax(a.x, w.soft, a.rows, a.n, nullptr, st)) return rc; }
            else for (int r = 0; r < a.rows; ++r) if (int rc = mllm_hip_softmax(a.x + r * a.ld, w.soft + (int64_t)r * a.n, 1, a.n, nullptr, st)) return rc;
            src = w.soft; lds = a.n;
        }
        // std::sort of the whole (score, index) row: mllm_hip_sort_desc per row (the device-wide radix sort, which uses the chip for one row)
        for (int r = 0; r < a.rows; ++r)
            if (int rc = mllm_hip_sort_desc(src + r * lds, a.n, w.val + (int64_t)r * a.n, w.idx + (int64_t)r * a.n, w.sort, w.sort_bytes, st)) return rc;
        t.n_cand = a.n; t.nucleus = 1;
    }
    t.val = w.val; t.idx = w.idx; t.ldc = w.ldc; t.prob = w.prob;
    t.top_p = a.top_p; t.temperature = a.temperature; t.ctl = a.ctl;
    t.u01 = a.u01; t.seqs = a.seqs; t.cap = a.cap;
    t.ids_out = a.ids_out; t.cand_idx = a.cand_idx; t.cand_prob = a.cand_prob; t.cand_ld = a.cand_ld; t.cand_n = a.cand_n;
    t.n_ambiguous = a.n_ambiguous;
    hipLaunchKernelGGL(sample_tail_kernel, dim3(a.rows), dim3(TAIL_NT), 0, st, t);
    return MH_LAUNCH_OK("sample_tail");
}
int seqs_sample_next_launch(const int *drawn, int B, int cap, SeqKV *seqs_dev, BatchCtl *ctl, int *tok_out, float *ids_f, int *history, int hist_ld, hipStream_t st) {
    if (B < 1 || B > 64) return MLLM_HIP_ERR_SHAPE;
    hipLaunchKernelGGL(seqs_sample_next_kernel, dim3(1), dim3(64), 0, st, seqs_dev, ctl, drawn, B, cap, tok_out, ids_f, history, hist_ld);
    return MH_LAUNCH_OK("seqs_sample_next");
}
}  // namespace mllm_hip

extern "C" size_t mllm_hip_sample_rows_workspace_bytes(int rows, int n, int method, int top_k) { return sample_rows_workspace_bytes(rows, n, method, top_k); }
extern "C" int mllm_hip_sample_rows(const float *x, int64_t ld, int rows, int n, int method, int top_k, float top_p, float temperature, int softmax_first, const float *u01,
                                    int *ids_out, int *cand_idx, float *cand_prob, int64_t cand_ld, int *cand_n, int *n_ambiguous, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    SampleRows a{};
    a.x = x; a.ld = ld; a.rows = rows; a.n = n; a.method = method; a.top_k = top_k; a.softmax_first = softmax_first;
    a.top_p = top_p; a.temperature = temperature; a.u01 = u01;
    a.ids_out = ids_out; a.cand_idx = cand_idx; a.cand_prob = cand_prob; a.cand_ld = cand_ld; a.cand_n = cand_n; a.n_ambiguous = n_ambiguous;
    a.ws = workspace; a.ws_bytes = workspace_bytes;
    return sample_rows_launch(a, as_stream(stream));
}

// ---- the one exchange step of the sharded vision prefill ------------------------------------------------------------------------------
extern "C" int mllm_hip_comm_unique_id(void *id128) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    if (!id128) return MLLM_HIP_ERR_ARG;
    return ncclGetUniqueId((ncclUniqueId *)id128) == ncclSuccess ? MLLM_HIP_OK : MLLM_HIP_ERR_HIP;
}
extern "C" int mllm_hip_comm_create(const void *id128, int world, int rank, void **comm) {
    if (!id128 || !comm || world <= 0 || rank < 0 || rank >= world) return MLLM_HIP_ERR_ARG;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t c;
    if (ncclCommInitRank(&c, world, id, rank) != ncclSuccess) return MLLM_HIP_ERR_HIP;
    *comm = (void *)c;
    return MLLM_HIP_OK;
}
extern "C" int mllm_hip_comm_destroy(void *comm) {
    if (!comm) return MLLM_HIP_ERR_ARG;
    return ncclCommDestroy((ncclComm_t)comm) == ncclSuccess ? MLLM_HIP_OK : MLLM_HIP_ERR_HIP;
}
extern "C" int mllm_hip_all_gather_rows(void *comm, const float *local_dev, float *all_dev, int64_t rows_per_rank, int cols, void *stream) {
    if (!comm || !local_dev || !all_dev || rows_per_rank < 0 || cols <= 0) return MLLM_HIP_ERR_ARG;
    if (rows_per_rank == 0) return MLLM_HIP_OK;
    return ncclAllGather(local_dev, all_dev, (size_t)rows_per_rank * cols, ncclFloat, (ncclComm_t)comm, as_stream(stream)) == ncclSuccess ? MLLM_HIP_OK : MLLM_HIP_ERR_HIP;
}

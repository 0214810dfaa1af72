// mllm_amd/csrc/decode_launch.h -- host-side description of one fused decode step (kernels_decode.hip), used by engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

namespace mllm_hip {

// per-step scalars in device memory, advanced by dec_next_kernel so one captured graph replays every step
struct DecodeState {
    int T;      // tokens already in the KV slab before this step
    int step;   // decode step since the prefill (row of the rotary tables)
    int token;  // token id to embed at this step
    int serial; // steps since the state was armed: the epoch of the in-launch hand-offs (merged attention + o-projection launch)
};

struct DecodeLayer {
    const float *in_norm, *post_norm;
    const uint8_t *Wqkv; const float *bqkv; int qkv_N;
    const uint8_t *Wo, *Wgu, *Wdown;          // all four in decode order (decode_order_q4k)
    const uint8_t *Wgu_raw, *Wdown_raw, *Wo_raw;       // the rows as stored on disk (the one-lane-per-super-block kernels dec_gateup_blk / dec_proj_blk)
};

// Weights the kernels behind the attention launch will stream, touched by workgroups the attention does not need (24 of 256 CUs hold a head): region r is read by the
// later launch's workgroup g as [base[r] + g * bytes[r], + bytes[r]); the warming workgroup with blockIdx % 8 == g % 8 runs on the XCD whose L2 that workgroup will read
// (consecutive launches place blockIdx b on XCD b % 8).  n == 0: off.  A speed matter only.
struct WeightWarm {
    static constexpr int MAXR = 4, GROUPS = 32;      // targets per XCD column: 8 x 32 = 256 workgroups of the later launches
    const uint8_t *base[MAXR];
    int bytes[MAXR], count[MAXR], n;
    uint32_t *sink;
};

struct DecodeCtx {
    DecodeState *state;
    int H, I, heads, kv_heads, D, vocab, cache_limit, nsplit, max_parts;
    float eps, final_eps;
    const uint8_t *emb_qs; const uint16_t *emb_d; const float *final_norm;
    const uint8_t *Whead;               // Linear lm_head rows (Q4_K, decode order) when the head is not tied to embed_tokens, else nullptr
    float *x0, *x1, *qkv, *act, *logits, *fa_ws, *part_val, *normed;
    int8_t *x80_qs; uint16_t *x80_d;
    int *part_idx, *tok_dev, *history;
    const float *rope_sin, *rope_cos;   // [cache_limit][D/2], row = DecodeState::step
    float *cur_sin, *cur_cos;           // [D/2]: the row of the step about to run (refreshed by dec_next)
    uint16_t *kslab, *vslab;            // K: [layers][cache_limit][Hkv*D]; V transposed: [layers][Hkv*D][vt_ld]
    int vt_ld;
    int n_layers;                       // entries of the DecodeLayer array handed to the launchers
    const WeightWarm *warm_tab;         // device, [n_layers] (decode_warm_table), or nullptr: no warming workgroups in the attention launch
    // shared launches (StepPlan, option "merge_o"): the attention's output row travels as {value, epoch} pairs, one row per layer, epoch = DecodeState::serial;
    // the o-projection's workgroups ride in the attention's launch, fetch their weight rows at once and poll the pairs (profiles/r04_seam_overlap_microbench.md)
    unsigned long long *attn_pairs;     // [n_layers][heads * D], all-ones when the state is armed
    unsigned long long *x_pairs;        // [n_layers][H]: a layer's output row for the next layer's q|k|v role (and the o-projection's residual) when both ride in the down projection's launch (merge_o = 4)
    unsigned long long *qkv_pairs;      // [n_layers][(heads + 2 kv_heads) * D]: q | k | v for the attention role when the q|k|v projection rides in the same launch (merge_o = 3)
    int *poll_err;                      // set when a poll gave up (bounded spins): the step's results are then invalid and the host reports it
};

// ---- the step plan: the launches of one decode step in issue order, decided once per model (decode_step_plan, when the model is created) and issued from there ----
// A decoder layer is five kernels -- q|k|v, attention, o-projection, gate|up, down -- that run either as launches of their own or as roles of a shared launch: attention +
// o-projection (STEP_ATTN with o_rows != 0), q|k|v + attention + o-projection (STEP_FRONT), or a layer's down projection + the next layer's q|k|v + attention +
// o-projection (STEP_CHAIN; never layer 0's roles, whose q|k|v embeds the token).  The plan is the only place where a form is chosen: the launchers take the choice
// from a StepLaunch, the timing marks take its kind, the warming table asks o_in_attn.  It holds no device pointer, so it outlives a change of the KV slabs in DecodeCtx.
// The kinds of launch of a step (also what StepMarks reports and mllm_hip_model_time_step sums by): STEP_HEAD = model.norm + lm_head, STEP_NEXT = argmax / state advance
enum StepKind { STEP_QKV, STEP_ATTN, STEP_OPROJ, STEP_GATEUP, STEP_DOWN, STEP_CHAIN, STEP_FRONT, STEP_HEAD, STEP_NEXT, STEP_KINDS };
struct StepLaunch {
    int kind;       // a StepKind
    int layer;      // the layer of the launch's first role (STEP_CHAIN: the layer of the down projection; the other roles are layer + 1's); unused by STEP_HEAD, STEP_NEXT
    int persist;    // QKV, GATEUP, HEAD (Linear head): workgroups per CU of the walking / persistent grid, 0 = a workgroup per row group
    bool blk;       // OPROJ, DOWN: the lane-per-super-block projection dec_proj_blk; GATEUP: the lane-per-super-block dec_gateup_blk; false: the eight-lane kernels
    int ds;         // ATTN, CHAIN, FRONT: attention workgroups per head (the shared launches: 2)
    bool pipe;      // ATTN without the o-projection: the pipelined attention kernel (else dec_attn_kernel)
    int o_rows;     // rows per wave of the o-projection role: 1 in CHAIN and FRONT; ATTN: 1 under merge_o = 2, else 2, and 0 = no o-projection in the attention's launch
    int cont;       // CHAIN: the q|k|v role is carried on by the first down-projection workgroups (option chain_cont, and a q|k|v grid no larger than the down projection's)
    int head;       // HEAD: 0 Linear lm_head, 1 tied head by the stand-alone launchers, 2 tied head + partial argmax in one kernel
    int rows;       // HEAD (form 2): rows per wave
    int parts;      // HEAD (form 2): workgroups = partial maxima; NEXT: the partial maxima to fold, 0 = an argmax launch over the logits row comes first
    size_t lds;     // ATTN (pipelined or with the o-projection), CHAIN, FRONT: dynamic LDS bytes of the launch
};
// The launch-form options (merge_o, attn_flags, attn_ds, chain_cont, pjb_min_ns, no_pjb, no_gub, gu_persist, qkv_persist, head_wpc) are read by decode_step_plan and nowhere
// else: a later mllm_hip_set_option does not reach a live model.  What the plan keeps of them is what the engine and the launcher still need.
struct StepPlan {
    int merge_o;        // level asked for, 0..4 (default 4: chain; 3: front; 2: attention + o-projection; 1: that with two rows per wave; 0: five launches per layer).
                        // Non-zero: the engine arms the {value, epoch} pairs and checks poll_err, whichever forms the shapes then allowed
    int attn_flags;     // bit 0 XCD placement of a K/V group's heads, bit 1 two-stage key fetch (un-pipelined kernel), bit 2 keep the un-pipelined kernel, bit 3 the q|k|v
                        // projection warms the L2 with the cache rows, bits 4..7 weight-warming workgroups (decode_warm_table).  Default 91
    bool o_in_attn;     // every layer's o-projection rides in the launch of its attention (ATTN, CHAIN, FRONT): no STEP_OPROJ in the plan
    std::vector<StepLaunch> launches;      // the step
    std::vector<StepLaunch> alone;         // [n_layers][5]: kernel STEP_QKV .. STEP_DOWN of a layer as a launch of its own (what the step is made of where nothing merges,
                                           // and what mllm_hip_model_time_kernel times)
};
void decode_step_plan(const DecodeCtx &c, const DecodeLayer *layers, int n_layers, StepPlan *out);
int decode_launch(const DecodeCtx &c, const StepPlan &p, const DecodeLayer *layers, const StepLaunch &e, hipStream_t st);

// raw Q4_K rows -> decode order: the nibble dwords of every super-block transposed so that a lane's 16 bytes are one column class (q4k_dot.h)
int decode_order_q4k(const void *src, void *dst, int64_t n_blocks, hipStream_t st);
int decode_warm_table(const DecodeCtx &c, const DecodeLayer *layers, int n_layers, int flags, WeightWarm *host_out);
int argmax_row_launch(const DecodeCtx &c, const float *logits, int n, int *out, hipStream_t st);      // first-maximum argmax over the chip, partials in c.part_val / c.part_idx
// The step: a loop over the plan's launches.  Optional marks around every launch (mllm_hip_model_time_step: the step run eagerly with a HIP event either side of each
// launch); kind = the launch's StepKind.
struct StepMarks { int (*mark)(void *user, int kind, int after); void *user; };
int decode_step_launch(const DecodeCtx &c, const StepPlan &p, const DecodeLayer *layers, hipStream_t st, const StepMarks *marks = nullptr);

// ---- batched decode (engine.hip: mllm_hip_model_batch_decode / _batch_generate): the launches of a B-row step that are not row-wise Ops ----
// One sequence's state in device memory.  The kernels read it from there (never from kernel arguments), so a captured step neither bakes a sequence's slabs in nor
// needs the host between steps: seqs_next_kernel advances it.  The id to embed at the next step is not kept here: it lives as the fp32 id mllm_hip_embedding_q40 reads.
struct SeqKV {
    uint16_t *k; uint16_t *v;   // the sequence's KV slabs (bases of layer 0)
    int t;                      // tokens its cache holds BEFORE this step
    int pos;                    // rotary position of the token this step appends (row of the resident table; after an image prompt smaller than t)
    int active;                 // 0: stopped at the end-of-sequence id -- the step leaves its cache and counters alone
    int made;                   // steps made since the state was uploaded (the column of its history row)
};
// what the whole batch shares: the end-of-sequence id (< 0: none) and the rows still active after the last step (the host reads it every few steps)
struct BatchCtl { int eos; int n_active; };
// row b of qkv ([B][ldq]: q | k | v of sequence b's new token): q rotated in place, k rotated -> fp16 row t_b of sequence b's K slab, v -> column t_b of its transposed V slab
// (qkv_rope_append_kernel's arithmetic, S = 1 per sequence).  sin_t / cos_t: the resident table [tab_rows][ld_tab], row = the sequence's pos.  A stopped sequence, or one
// whose cache is full (t >= cap), is skipped.
int seqs_rope_append_launch(float *qkv, int64_t ldq, const float *sin_t, const float *cos_t, int ld_tab, int tab_rows, const SeqKV *seqs_dev, int64_t layer_k_off,
                            int64_t layer_v_off, int64_t ldk, int64_t ldvt, int B, int Hq, int Hkv, int D, int cap, hipStream_t st);
// __fa2_decode of row b's query over sequence b's t_b + 1 keys (fa2_decode_kernel's body, grid = heads x sequences); cap = the slabs' capacity in keys
int seqs_fa2_decode_launch(const float *q, int64_t ldq, const SeqKV *seqs_dev, int64_t layer_k_off, int64_t layer_v_off, int64_t ldk, int64_t ldvt, float *o, int64_t ldo, int B,
                           int Hq, int Hkv, int D, int cap, hipStream_t st);
// first-maximum argmax of the B logits rows and the state advance, two launches: partial maxima over (nparts, B) workgroups, then one workgroup (a wave per row) folds row
// b's partials, writes the id to tok_out[b], history[b][made_b] and ids_f[b] (the next step's embedding input), advances t / pos / made of the active rows and clears
// `active` on the end-of-sequence id.  part_val / part_idx hold B * nparts entries; B <= 16.
int seqs_argmax_next_launch(const float *logits, int64_t ld_logits, int vocab, int B, float *part_val, int *part_idx, int nparts, SeqKV *seqs_dev, BatchCtl *ctl, int *tok_out,
                            float *ids_f, int *history, int hist_ld, hipStream_t st);

// ---- batched sampling (kernels_sample.hip; engine.hip: mllm_hip_model_batch_generate_sampled): the sampled tail of a B-row step ----
// what a captured sampled step reads from device memory, so that another nucleus mass, temperature or number of steps needs no re-capture
struct SampleCtl {
    float top_p, temperature;
    int u_ld;            // uniform numbers per row of u01 (the call's steps)
    int n_ambiguous;     // candidates whose exp() lay within 2 double ulps of a float rounding tie (ref_arith.h f32_rounding_ambiguous): the engine's counter, which
                         // it hands to the launcher as SampleRows::n_ambiguous like any other caller
};
// mllm_hip_sample_rows (include/mllm_hip.h) with everything a captured step needs: ctl != nullptr: top_p / temperature / u_ld are read from it (and from nowhere else);
// n_ambiguous is the one counter the kernels add to (nullptr: none); seqs != nullptr: row b draws on u01[b * u_ld + made_b], and a row that has stopped or whose cache is
// full (t >= cap) draws nothing.
struct SampleRows {
    const float *x; int64_t ld; int rows, n, method, top_k, softmax_first;
    float top_p, temperature; const SampleCtl *ctl;
    const float *u01; const SeqKV *seqs; int cap;
    int *ids_out; int *cand_idx; float *cand_prob; int64_t cand_ld; int *cand_n; int *n_ambiguous;
    void *ws; size_t ws_bytes;
};
size_t sample_rows_workspace_bytes(int rows, int n, int method, int top_k);
int sample_rows_launch(const SampleRows &a, hipStream_t st);
// seqs_next_kernel with the drawn id in place of the folded argmax: drawn[b] -> tok_out[b], history[b][made_b], ids_f[b]; t / pos / made of the active rows advance,
// `active` is cleared on the end-of-sequence id, BatchCtl::n_active counted.  A row whose cache is full (t >= cap) is left alone, like a stopped one.
int seqs_sample_next_launch(const int *drawn, int B, int cap, SeqKV *seqs_dev, BatchCtl *ctl, int *tok_out, float *ids_f, int *history, int hist_ld, hipStream_t st);
// kernels_elem.hip, rows in blockIdx.y, scratch from the caller (capturable): the k best of every row in mllm_hip_topk's order; the long-row softmax of mllm_hip_softmax
size_t rows_topk_scratch_bytes(int rows, int n, int k);
int rows_topk_launch(const float *x, int64_t ld, int rows, int n, int k, float *out_val, int *out_idx, int ldo, void *scr, hipStream_t st);
size_t softmax_long_rows_scratch_bytes(int rows, int n);
int softmax_long_rows_launch(const float *x, int64_t ldx, float *y, int64_t ldy, int rows, int n, float *scr, hipStream_t st);

// ---- batched prefill (engine.hip: mllm_hip_model_batch_prefill): the prompts of B sequences sit concatenated, sequence after sequence, in the activation buffers ----
// One sequence's share of the pass.  The host knows every length, fills the array and uploads it once per call; the kernels read it from device memory.
struct PrefillSeq {
    uint16_t *k; uint16_t *v;   // the sequence's KV slabs (bases of layer 0)
    int row0;                   // its first row in the concatenated buffers (and in the concatenated rotary table)
    int S;                      // its prompt rows
    int T0;                     // tokens its cache holds before the call
    int Sk;                     // T0 + S: the keys its last row sees
    int sk_eff;                 // the key columns the reference's tiling walks (launch_fa2: Tc = Sk / 4, Tc * 4 + (Tc ? Sk % Tc : 0) for fp16 K / V)
    int pad;
};
// one query row of a sequence with fewer than four prompt rows: the reference's Br = Bc = 1 recurrence, the decode walk of row `row` over keys 0 .. t
struct PrefillRow { uint16_t *k; uint16_t *v; int t; int row; };
// rows [row0, row0 + S) of qkv: q rotated in place, k rotated -> fp16 rows T0 .. T0 + S - 1 of the sequence's K slab, v -> columns T0 .. of its transposed V slab
// (qkv_rope_append_kernel's arithmetic); row r takes row r of the concatenated table.  One launch for all B sequences; max_S = the longest S (sizes the grid).
// The host has checked T0 + S <= the slabs' capacity for every sequence.
int prefill_seqs_rope_append_launch(float *qkv, int64_t ldq, const float *sin_t, const float *cos_t, int ld_tab, const PrefillSeq *seqs_dev, int64_t layer_k_off,
                                    int64_t layer_v_off, int64_t ldk, int64_t ldvt, int B, int max_S, int Hq, int Hkv, int D, hipStream_t st);
// causal __fa2_prefill_append (Br = Bc = 4) of every sequence with S >= 4 in one launch: fa2_prefill_kernel<D, true, true>'s body, blockIdx.z = sequence, its rows, slabs
// and key counts read from its descriptor; a sequence with S < 4 is left to prefill_rows_fa2_decode_launch.  D = 64 or 128.
int prefill_seqs_fa2_launch(const float *q, int64_t ldq, const PrefillSeq *seqs_dev, int64_t layer_k_off, int64_t layer_v_off, int64_t ldk, int64_t ldvt, float *o, int64_t ldo,
                            int B, int max_S, int Hq, int Hkv, int D, hipStream_t st);
// __fa2_decode of n_rows single query rows, each over its own sequence's keys 0 .. t (fa2_decode_seqs_kernel's body, the row's place in q / o read from its descriptor)
int prefill_rows_fa2_decode_launch(const float *q, int64_t ldq, const PrefillRow *rows_dev, int64_t layer_k_off, int64_t layer_v_off, int64_t ldk, int64_t ldvt, float *o,
                                   int64_t ldo, int n_rows, int Hq, int Hkv, int D, int cap, hipStream_t st);
// dst[b][:] = src[rows[b]][:] for b < B (the last row of every sequence, gathered for the head); dim a multiple of 4
int gather_rows_launch(const float *src, const int *rows_dev, float *dst, int B, int dim, hipStream_t st);
// B first-maximum argmaxes (std::max_element per row) -> tok_out[b]; part_val / part_idx hold B * nparts entries
int rows_argmax_launch(const float *logits, int64_t ld_logits, int vocab, int B, float *part_val, int *part_idx, int nparts, int *tok_out, hipStream_t st);

}  // namespace mllm_hip

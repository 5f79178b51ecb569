/*
 * parrot_hip.h -- C ABI of libparrot_hip.so, the MI355X (gfx950) implementation of the
 * acoustic-frame generation hot path of sotelo/parrot (Char2Wav).
 *
 * The reference has no FFI boundary of its own: the hot path sits behind Python brick/operator
 * calls that Theano compiles at run time.  Each entry point below names
 * the reference call it replaces (file:line relative to the reference checkout).  The Python host
 * layer (parrot_amd/) binds these symbols with ctypes; INTEGRATION.md shows the stub a maintainer
 * of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - matrices are row-major float32 with explicit leading dimensions, "x . W" convention of the
 *     reference (W is [in, out]);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it, the
 *     library never synchronises and never allocates device memory;
 *   - return value 0 = success; otherwise a hipError_t value, or PARROT_ERR_* for bad arguments.
 *     Plans additionally keep the first error (parrot_plan_last_error).
 */
#ifndef PARROT_HIP_H
#define PARROT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PARROT_ERR_BADARG 10001
#define PARROT_ERR_UNSUPPORTED 10002

#define PARROT_NORM_EPS 1e-5f /* _simple_norm's eps default, model.py:24 */
#define PARROT_MAX_LAYERS 3

/* Library / build identification ("parrot_hip <ver> gfx950"). */
const char* parrot_hip_version(void);

/* Measurement aid (bench.py roofline leg): between begin and end every dispatch of the recurrent-step
 * kernel is timed with HIP events attached to the dispatch (hipExtLaunchKernelGGL start/stop events)
 * and its algorithmic flops / bytes are accumulated.  Use only with eager plans (use_graph = 0) and
 * call parrot_profile_end after synchronising the stream; it returns the number of dispatches and the
 * summed kernel time [us], flops and bytes. */
int parrot_profile_begin(void);
long long parrot_profile_end(double* total_us, double* flops, double* bytes);
/* As parrot_profile_end; plain4 (or NULL) receives {dispatch time in us, flops, bytes, launch count} of the PLAIN step-GEMM
 * launches alone (no attention / state row blocks in the grid): the dominant kernel without the latency chains that the
 * heterogeneous launches carry beside their GEMM workgroups. */
long long parrot_profile_end2(double* total_us, double* flops, double* bytes, double* plain4);

/* ------------------------------------------------------------------------------------------
 * Dense projections (Blocks Linear / Fork applies, model.py:580-627, 739-755; lib.ops.Linear,
 * sampleRNN/lib/ops.py:32-128).  C[M,N] (+)= alpha * opA(A) * opB(B) + bias, f32 MFMA.
 *   transA = 0: A is [M,K] (lda), 1: A is stored [K,M] (lda)      (same for B / transB, [K,N])
 *   batched with element strides; split_k > 1 splits K over workgroups, the partial products are summed in
 *   slice order by a second kernel (deterministic; inside a stream capture the product runs unsplit);
 *   split_k = 0 picks a split automatically (long reductions with few output tiles, e.g. deferred weight gradients).
 *
 * Small-M dispatch: a call with M <= 64, transA = 0, nbatch = 1, split_k <= 1, alpha = 1 and no gate runs on the
 * weight-streaming recurrent-step kernel (f32 operands whatever the precision mode).  Any one of alpha != 1, a gate
 * (parrot_gemm_gated), split_k > 1, transA = 1 or nbatch > 1 keeps a product of any M on the batched kernels below.
 *
 * accumulate together with an activation (act != 0) is rejected with PARROT_ERR_BADARG on every path: the step kernel
 * would add C after the activation and the batched kernels before it, so the meaning would change between M = 64 and
 * M = 65.  split_k > 1 with an activation is rejected too (the automatic rule never splits such a product).
 * ------------------------------------------------------------------------------------------ */
#define PARROT_PRECISION_F32 0
#define PARROT_PRECISION_BF16 1
#define PARROT_PRECISION_BF16X3 2
/* Operand precision of the batched kernels of parrot_gemm / parrot_gemm_gated (every call the small-M rule above does
 * not send to the step kernel), process-wide:
 *   PARROT_PRECISION_BF16X3 (the default; PARROT_GEMM_PRECISION=f32 / bf16 in the environment picks another): f32
 *     operands, each split into three bf16 terms inside the kernel, six bf16 matrix instructions per block, f32
 *     accumulation: f32-grade results at 1.7-1.9 x the rate of the f32-input kernel.  It covers the products that are
 *     eligible: no activation or relu, M >= 128, N >= 128, K >= 64, both operand pointers 16-byte aligned, lda, ldb and
 *     both batch strides multiples of 4, and the contiguous extent of each operand (K, or M for transA; N, or K for
 *     transB) a multiple of 4.  Every other product (tanh / sigmoid epilogues included) runs as under
 *     PARROT_PRECISION_F32.
 *   PARROT_PRECISION_F32: the f32-input matrix instructions for everything (the reference computes in floatX =
 *     float32, model.py:21).
 *   PARROT_PRECISION_BF16: A and B are read as f32 and rounded to bf16 (nearest even) on their way into the matrix
 *     cores, products are accumulated in f32, C / bias / activation stay f32 (BASELINE configs[3]).
 * Not a per-stream setting: change it only between calls.  A decoder plan created with bf16 = 1 applies the bf16 mode
 * to its own batched projections regardless. */
int parrot_set_gemm_precision(int mode);
int parrot_get_gemm_precision(void);
int parrot_gemm(const float* A, int lda, int transA, const float* B, int ldb, int transB, float* C, int ldc,
                int M, int N, int K, const float* bias, float alpha, int accumulate, int act, int nbatch,
                long long strideA, long long strideB, long long strideC, int split_k, void* stream);

/* C[M,N] = A . B kept where gate[m,n] > 0 and zeroed elsewhere (gate: row-major, leading dimension ldg >= N): the
 * backward of y = relu(x . W + b) through the saved activation y, fused into the product that makes the gradient wrt
 * relu's output (three_tier.py:504-509: the two ReLU layers of sample_level_predictor).  Operand layouts as parrot_gemm. */
int parrot_gemm_gated(const float* A, int lda, int transA, const float* B, int ldb, int transB, float* C, int ldc,
                      int M, int N, int K, const float* gate, int ldg, void* stream);

/* Which kernel a parrot_gemm call with these arguments takes under the precision mode now in effect, and how many K
 * slices it plans (has_gate != 0: a parrot_gemm_gated call; pass alpha = 1, act = 0, nbatch = 1, split_k = 0 as it
 * does).  A and B are only inspected for their alignment, never dereferenced; no HIP call is made, so the query works
 * without a device.  *slices is the planned count (split_k if > 0, else the automatic rule), before the fallback to
 * one slice inside a stream capture or without a workspace; it is 1 for the step kernel.  Returns PARROT_ERR_BADARG for
 * arguments parrot_gemm rejects (null pointers, extents < 1, a batched gate, an activation with more than one slice). */
#define PARROT_GEMM_ROUTE_STEP 0   /* sk_kernel */
#define PARROT_GEMM_ROUTE_F32 1    /* bg_kernel8 */
#define PARROT_GEMM_ROUTE_BF16 2   /* bg_kernel_bf16 */
#define PARROT_GEMM_ROUTE_BF16X3 3 /* bgs_kernel */
int parrot_gemm_route(const float* A, int lda, int transA, const float* B, int ldb, int transB, int M, int N, int K,
                      float alpha, int act, int nbatch, long long strideA, long long strideB, int split_k, int has_gate,
                      int* kernel, int* slices);

/* How the host lays out one step-kernel launch of njobs (1..9) jobs (introspection, as parrot_gemm_route; no HIP call is
 * made, so the query works without a device).  Job q has M[q] rows, N[q] output columns and one K[q]-deep operand
 * segment (K % 16 != 0 puts the job on the generic path, which keeps the whole launch on one column tile per
 * workgroup); lstm_H (or NULL) > 0 marks an LSTM-cell job with N = 4 * lstm_H gate-interleaved columns.  info gets
 * 5 + njobs values: {z-mode 0/1, 10 * MB + NB (row and column blocks of 16 per workgroup), grid.x, grid.y, grid.z,
 * then per job the number of workgroups along x up to and including that job}.  z-mode = every job has the same number
 * of workgroups: grid.z enumerates the jobs and the kernel instantiation that never reads the launch header runs;
 * otherwise the jobs lie back to back along x and the kernel finds its job in that prefix table.  The wide bf16 kernel,
 * which takes some bf16-operand launches instead, is not part of the query. */
int parrot_step_launch_mode(int njobs, const int* M, const int* N, const int* K, const int* lstm_H, int* info);

/* ONE step-kernel job as one launch of its own (the scan plans build their launches themselves; this is the kernel alone,
 * for tests and probes): acc[M, N] = sum over nseg (1..5) K segments of A[s][M, K[s]] (row-major, leading dimension
 * lda[s]) times the segment's weights, then the epilogue `epi`.  layout, one for all segments: 0 = B[s][k * ldb + n],
 * 1 = B[s][n * ldb + k], 2 = fragment-major copy (parrot_tile_weights; ldb[s] = floats between consecutive column tiles
 * = K[s] / 16 * 256), 3 = its bf16 twin (parrot_tile_weights_bf16; ldb[s] = K[s] / 32 * 256, counted in 4-byte units).
 * M <= 64 rows per 64-row grid row as in the plans; force_tile = 10 * MB + NB asks for (16 MB) x (16 NB) tiles where
 * legal (0: the host's choice).  Epilogues (every cell buffer [M, H] with leading dimension H):
 *   0 linear:     out[M, N] (ld ldo) (+)= act(acc + bias + add)   (accumulate adds the prior content AFTER act)
 *   1 GRU gates:  N = 2 H: z = sigmoid(.) -> o1, r = sigmoid(.) -> o2, r * e0 (h_prev) -> out
 *   2 GRU cand.:  N = H:   c = tanh(.) -> o1 (or NULL), e1 (z) * c + (1 - e1) * e0 (h_prev) -> out
 *   3 backward:   N = H:   acc = d(r * h_prev): acc * e0 (h_prev) * e1 (r) * (1 - e1) -> out (ld ldo), o1 += acc * e1
 *   4 LSTM cell:  N = 4 H gate-interleaved columns: activations -> o2 [M, 4H] (or NULL), e1 (c_prev) * f + g * i -> o1,
 *                 tanh(o1) * o -> out
 * bias [N] and add [M, N] (ld ld_add) may be NULL. */
int parrot_step_job(int epi, int M, int N, int H, int nseg, const float* const* A, const int* lda, const void* const* B,
                    const int* ldb, const int* K, int layout, int act, int accumulate, int force_tile, const float* bias,
                    const float* add, int ld_add, float* out, int ldo, const float* e0, const float* e1, float* o1, float* o2,
                    void* stream);

/* bf16-IN weight-gradient product (round 4): C[M,N] (+)= A^T . B with A [K, M] and B [K, N] ALREADY bf16 in device
 * memory (row-major, leading dimensions in elements, both multiples of 8; M, N multiples of 8; 16-byte aligned),
 * f32 accumulation, f32 C; deterministic split-K as parrot_gemm (split_k = 0: automatic).  parrot_to_bf16 makes the
 * operand copies (round to nearest even, n a multiple of 8): what a bf16-operand decoder's deferred weight gradients
 * dW = X^T . dPre (the Theano gradient of the Fork / recurrent weights inside model.py:651-724) run on. */
int parrot_to_bf16(const float* x, void* y, long long n, void* stream);
int parrot_gemm_bf16in(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                       int accumulate, int split_k, void* stream);
/* Round 5: the same bf16-in product for every operand layout parrot_gemm takes (A(m,k) at A[m*lda + k], or A[k*lda + m]
 * when transA; B(k,n) at B[k*ldb + n], or B[n*ldb + k] when transB; leading dimensions in bf16 elements, multiples of 8;
 * K % 8 == 0; the contiguous extent of an operand a multiple of 8), plus an optional f32 bias [N]: the readout products
 * h . Wr and dread . Wr^T of a bf16-operand decoder (model.py:739-755) on bf16 copies instead of f32 operands rounded
 * inside the product.  parrot_gemm_bf16in(A, ...) == parrot_gemm_bf16in_ex(A, lda, 1, B, ldb, 0, ..., NULL, ...). */
int parrot_gemm_bf16in_ex(const void* A, int lda, int transA, const void* B, int ldb, int transB, float* C, int ldc, int M,
                          int N, int K, const float* bias, int accumulate, int split_k, void* stream);

/* out[n] (+)= sum_m x[m, n]  -- bias gradients. */
int parrot_colsum(const float* x, long long M, int N, int ld, float* out, int accumulate, void* stream);
/* Which kernel a parrot_colsum call with these arguments takes and how many row slices it plans (introspection, as
 * parrot_gemm_route): info2 = {0 colsum_kernel (one column per lane) / 1 colsum4_kernel (four columns per lane: N and ld
 * multiples of 4, x and out 16-byte aligned, M >= 64), row slices}.  More than one slice: the kernel writes partial sums
 * and colsum_finish_kernel adds them in slice order.  x and out are only inspected for their alignment, never
 * dereferenced (out = NULL: an aligned result); no HIP call is made, so the query works without a device.  The plan is
 * the one outside stream capture; inside a capture there is no partial buffer and the scalar kernel runs unsplit
 * wherever more than one slice is planned.  Returns PARROT_ERR_BADARG for x or info2 NULL, M < 0 or N < 1. */
int parrot_colsum_route(const float* x, long long M, int N, int ld, const float* out, int* info2);

/* ------------------------------------------------------------------------------------------
 * One GatedRecurrent step (Blocks GatedRecurrent.apply(inputs, gate_inputs, states,
 * iterate=False), model.py:659-662, 707-710, 719-722; same algebra ops.py:364-393):
 *   g = sigmoid(h . Wg + gate_inputs); z = g[:, :H]; r = g[:, H:]
 *   c = tanh((r*h) . Wc + inputs);     h' = z*c + (1-z)*h;  h' = m*h' + (1-m)*h if mask
 * Wg = state_to_gates [H,2H], Wc = state_to_state [H,H].  z, r, rh, c ([B,H] each) are the saved
 * activations the backward step needs.
 * ------------------------------------------------------------------------------------------ */
int parrot_gru_step_fwd(const float* h, const float* inputs, const float* gate_inputs, const float* mask,
                        const float* Wg, const float* Wc, float* h_out, float* z, float* r, float* rh,
                        float* c, int B, int H, void* stream);

/* Backward of the step: given dh_out [B,H] produces d_inputs (=dC) [B,H], d_gate_inputs (=dG)
 * [B,2H] and dh [B,H] (overwritten).  Weight gradients are left to the caller:
 * dWg += h^T dG, dWc += rh^T dC (parrot_gemm with transA = 1). */
int parrot_gru_step_bwd(const float* dh_out, const float* h, const float* mask, const float* Wg,
                        const float* Wc, const float* z, const float* r, const float* c, float* dh,
                        float* d_inputs, float* d_gate_inputs, int B, int H, void* stream);

/* ------------------------------------------------------------------------------------------
 * Plain GRU scans (Blocks GatedRecurrent.apply over a sequence -- the bidirectional encoder,
 * model.py:226-231, 245; lib.ops.LowMemGRU / stackedGRU, ops.py:395-440, 612-777).
 * Up to 4 independent chains (e.g. forward + backward direction) advance in the same launches.
 *
 * Indexing.  A chain's s-th processed step consumes time t = s (reverse: t = T-1-s).  The states h and their
 * gradients dh are indexed by SLOT (slot s+1 = after step s); everything else -- inputs, gate_inputs, mask, the saved
 * activations z / r / rh / c, and the gradients dG / dC -- is indexed by TIME t, also for a reversed chain.  (So the
 * weight gradients dWc += rh^T dC pair equal indices, while dWg += h[slot s]^T dG[t(s)] needs the flip.)
 * inputs[ch] / gate_inputs[ch] may be NULL: the chain then runs as if that operand were all zeros, and nothing is
 * read through the pointer.  dC / dG are written either way.
 * ------------------------------------------------------------------------------------------ */
typedef struct ParrotGruSeqDesc {
    int T, B, H, nchain, use_graph, reserved;
    int reverse[4];              /* chain consumes its inputs from t = T-1 down to 0 */
    const float* Wg[4];          /* [H,2H] */
    const float* Wc[4];          /* [H,H]  */
    const float* inputs[4];      /* [T,B,H]  pre-projected candidate inputs (biases included), or NULL = zeros */
    const float* gate_inputs[4]; /* [T,B,2H] or NULL = zeros */
    const float* mask;           /* [T,B] or NULL (shared by all chains) */
    float* h[4];                 /* [T+1,B,H]; slot 0 = initial state (caller), slot s+1 = state after
                                    the chain's s-th processed step */
    float* z[4]; float* r[4]; float* rh[4]; float* c[4]; /* [T,B,H] saved activations (indexed by time t) */
    /* backward */
    float* dh[4];                /* [T+1,B,H] in: dL/dh[slot] from consumers (slots 1..T), slot 0 zero;
                                    out: total gradient per slot (slot 0 = grad of the initial state) */
    float* dG[4];                /* [T,B,2H] out: gradient wrt gate_inputs (indexed by time t) */
    float* dC[4];                /* [T,B,H]  out: gradient wrt inputs      (indexed by time t) */
} ParrotGruSeqDesc;

int parrot_gru_seq_create(const ParrotGruSeqDesc* desc, void** plan);
int parrot_gru_seq_fwd(void* plan, void* stream);
int parrot_gru_seq_bwd(void* plan, void* stream);
int parrot_gru_seq_destroy(void* plan);

/* Which path a plan's scans take (introspection, as parrot_gemm_route): info4 = {row-wise 0/1, waves per 16-row block
 * (4 or 8; 0 on the launch path), H / 16 (0 on the launch path), reason}.  Row-wise = one launch per direction for the
 * whole sequence (rowgru.hip); otherwise the per-step launches, for the reason given.  Decided once, at create. */
#define PARROT_GRU_ROUTE_ROWWISE 0   /* reason: none, the plan is row-wise */
#define PARROT_GRU_ROUTE_SHAPE 1     /* H > 128 or H % 16 != 0 (parrot_gru_seq_rowwise_supported) */
#define PARROT_GRU_ROUTE_SWITCH 2    /* PARROT_GRU_ROWWISE=0 */
#define PARROT_GRU_ROUTE_UNALIGNED 3 /* a Wg / Wc pointer that is not 16-byte aligned */
#define PARROT_GRU_ROUTE_ALLOC 4     /* no memory for the fragment-major weight copies */
int parrot_gru_seq_route(void* plan, int* info4);
/* 1 if the row-wise kernels take the shape (T, B >= 1, H a multiple of 16 up to 128, 1..4 chains); needs no device. */
int parrot_gru_seq_rowwise_supported(int T, int B, int H, int nchain);

/* ------------------------------------------------------------------------------------------
 * LSTM scans (lib.ops.__LSTMStep / LowMemLSTM / stackedLSTM, sampleRNN/lib/ops.py:461-610, 823-989):
 *   pre = s_{t-1} . W + pre_in[t]   (pre_in = x_t . U + b, gate order i | f | o | g, each H wide)
 *   i,f,o = sigmoid, g = tanh;  c_t = c_{t-1}*f + g*i;  s_t = tanh(c_t)*o
 * W = Recurrent_Gates [H,4H].  s / c histories have T+1 slots (slot 0 = initial state).
 * Backward: in dS [T+1,B,H] (gradient wrt s slots from the consumers), in/out dc [B,H] (carry: gradient
 * wrt the final cell on entry, wrt the initial cell on return); out dP [T,B,4H] (gradient wrt pre_in) and
 * dS slot 0 (gradient wrt the initial state).  dW = s[0:T]^T dP is left to the caller (parrot_gemm).
 * ------------------------------------------------------------------------------------------ */
typedef struct ParrotLstmSeqDesc {
    int T, B, H, use_graph;
    const float* W;        /* [H,4H] */
    const float* pre_in;   /* [T,B,4H] */
    float* s; float* c;    /* [T+1,B,H] */
    float* gates;          /* [T,B,4H] saved activations (i|f|o|g after the nonlinearity) */
    float* dS;             /* [T+1,B,H] */
    float* dc;             /* [B,H] */
    float* dP;             /* [T,B,4H] */
} ParrotLstmSeqDesc;

int parrot_lstm_seq_create(const ParrotLstmSeqDesc* desc, void** plan);
int parrot_lstm_seq_fwd(void* plan, void* stream);
int parrot_lstm_seq_bwd(void* plan, void* stream);
int parrot_lstm_seq_destroy(void* plan);

/* ------------------------------------------------------------------------------------------
 * GMM-window attention step (model.py:664-690; sampling variant :931-958).
 * att_type 0 = graves, 1 = softmax.  WattT = h1_to_att [alpha;beta;kappa] weights stored
 * TRANSPOSED, [3A,H] (row j = output j), so the per-row dot products read contiguous memory.
 * ------------------------------------------------------------------------------------------ */
int parrot_gmm_attention_fwd(const float* h1, const float* WattT, const float* batt, const float* kappa_prev,
                             const float* ctx, float* a, float* b, float* kappa, float* phi, float* w, int B,
                             int H, int A, int U, int E, int att_type, float eps, float alignment,
                             float sharpening, float timing, void* stream);

/* dw [B,E] in; dkappa [B,A] in/out carry; dp [B,3A] out; dh1 [B,H] accumulated. */
int parrot_gmm_attention_bwd(const float* dw, const float* ctx, const float* a, const float* b,
                             const float* kappa, const float* kappa_prev, const float* WattT, float* dkappa,
                             float* dp, float* dh1, int B, int H, int A, int U, int E, int att_type, float eps,
                             void* stream);

/* The same two steps with the window's support handed from one to the other, as the training scan does: _fwd_sup also
 * writes sup [B,2] (int), the first / last context position whose window weight phi is not exactly 0 ((U, -1) when every
 * weight is 0, (0, U-1) under PARROT_ATT_DENSE=1); _bwd_sup reads it (null: as parrot_gmm_attention_bwd) and skips the
 * context rows outside it.  Same results as the plain entry points, bit for bit. */
int parrot_gmm_attention_fwd_sup(const float* h1, const float* WattT, const float* batt, const float* kappa_prev,
                                 const float* ctx, float* a, float* b, float* kappa, float* phi, float* w, int B,
                                 int H, int A, int U, int E, int att_type, float eps, float alignment,
                                 float sharpening, float timing, int* sup, void* stream);
int parrot_gmm_attention_bwd_sup(const float* dw, const float* ctx, const float* a, const float* b,
                                 const float* kappa, const float* kappa_prev, const float* WattT, float* dkappa,
                                 float* dp, float* dh1, int B, int H, int A, int U, int E, int att_type, float eps,
                                 const int* sup, void* stream);

/* Which path the attention backward row block takes for a batch row whose saved support is [u_lo, u_hi] (introspection,
 * as parrot_gemm_route; host arithmetic only): *route = 1 narrow (support present, 0 <= u_lo <= u_hi < U, at most
 * PARROT_ATT_BWD_CAP rows wide, U <= 256, E <= 256, PARROT_ATT_BWD_NARROW not 0: only the support's context rows are
 * fetched and reduced, the projection column is requested at entry), 0 wide (everything else; has_sup = 0: no support
 * handed in).  Both paths give the same bits. */
#define PARROT_ATT_BWD_CAP 64
int parrot_att_bwd_route(int U, int E, int has_sup, int u_lo, int u_hi, int* route);

/* ------------------------------------------------------------------------------------------
 * Whole-window decoder scan for training: the theano.scan over `step` of Parrot.compute_cost
 * (model.py:651-737) and its reverse-mode gradient.  L in {1,2,3} GRU layers with the reference's
 * dense skip topology (h_j -> h_l for j < l), attention after layer 1 (0-based layer 0).
 *
 * Packed per-layer weights, rows in this order (K_l = H + E + l*H, l 0-based):
 *     [ h_l (recurrent) ; w (attention context) ; h_0 .. h_{l-1} ]
 *   Wg[l] [K_l, 2H]: rnn{l+1}.state_to_gates ; inp_to_h{l+1}.gates ; h{j+1}_to_h{l+1}.gates
 *   Wc[l] [K_l,  H]: rnn{l+1}.state_to_state ; inp_to_h{l+1}.inputs ; h{j+1}_to_h{l+1}.inputs
 *   bg[l] [2H], bc[l] [H]: sums of the biases of the Forks feeding the layer.
 * Layer 0 consumes w_{t-1}; layers >= 1 consume w_t (model.py:655, 692-693).
 * History buffers have T+1 slots: slot 0 = state entering the window (learned initial state or the
 * carried last_* state, model.py:633-643), slot t+1 = value after step t.
 * ------------------------------------------------------------------------------------------ */
typedef struct ParrotDecoderDesc {
    int T, B, H, E, A, U, L, att_type, use_graph;
    int reserved; /* 0 (rounds 3-4: independent row "strands" on their own streams; measured slower, removed in round 5) */
    float eps, alignment, sharpening, timing;
    const float* Wg[PARROT_MAX_LAYERS];
    const float* Wc[PARROT_MAX_LAYERS];
    const float* bg[PARROT_MAX_LAYERS];
    const float* bc[PARROT_MAX_LAYERS];
    const float* WattT; /* [3A,H] */
    const float* batt;  /* [3A]   */
    const float* ctx;   /* [B,U,E] encoder output * labels_mask (model.py:645-646) */
    /* Per-step additive inputs (teacher-forcing feedback + speaker, model.py:562-627), or NULL.
     * For layers l >= 1 the buffers double as the destination of the chunk-batched projections of the lower
     * layers' outputs (see plans.hip, "chunked layer pipeline"): when every layer l >= 1 has them the scan
     * runs layer-pipelined and ADDS those projections in place (bit l of seq_init tells whether the buffer
     * holds caller data or is scratch to be overwritten).  The caller must refill them before each seq_fwd. */
    float* seq_c[PARROT_MAX_LAYERS]; /* [T,B,H]  */
    float* seq_g[PARROT_MAX_LAYERS]; /* [T,B,2H] */
    /* forward state / saved activations */
    float* h[PARROT_MAX_LAYERS];   /* [T+1,B,H] */
    float* w;                      /* [T+1,B,E] */
    float* kappa;                  /* [T+1,B,A] */
    float* z[PARROT_MAX_LAYERS]; float* r[PARROT_MAX_LAYERS];
    float* rh[PARROT_MAX_LAYERS]; float* c[PARROT_MAX_LAYERS]; /* [T,B,H] */
    float* a; float* b;            /* [T,B,A] */
    float* phi;                    /* [T,B,U] */
    /* backward */
    float* dh[PARROT_MAX_LAYERS];  /* [T+1,B,H] in: gradient from the readouts per slot (slot 0 included: it is added to).
                                      out: slot 0 = total wrt the state entering the window (plus dh_b[l][0] when given);
                                      slots s >= 1 = a partial sum: the total wrt h_l[s] is dh[l][s] + dhup[l][s]
                                      (+ dh_b[l][s] + dhup_b[l][s] + dhup_c[l][s] when given), which the state backward
                                      of step s-1 forms while it reads and never writes back */
    float* dw;                     /* [T+1,B,E] in: gradient from att_to_readout per slot; out: slots s >= 1 = total wrt
                                      w[s]; slot 0 keeps its in-value: the total wrt w[0] is dw[0] + dw0[0] (+ slot 0 of
                                      dw_b, dw_c, dw0_b, dw0_c when given) */
    float* dw0;                    /* [T+1,B,E] scratch, zero-filled by the caller: layer-0 share of dw */
    float* dhup[PARROT_MAX_LAYERS];/* [T+1,B,H] scratch, zero-filled by the caller: share of dh[l] that comes from
                                      the layers above (needed for l < L-1) */
    float* dkappa;                 /* [B,A] in: gradient wrt final kappa (0); out: wrt initial kappa */
    float* dG[PARROT_MAX_LAYERS];  /* [T,B,2H] out: gradient wrt gate pre-activations */
    float* dC[PARROT_MAX_LAYERS];  /* [T,B,H]  out: gradient wrt candidate pre-activations */
    float* dp;                     /* [T,B,3A] out: gradient wrt attention projection */
    /* LSTM variant of the layers (cell = 1; generalisation for BASELINE configs[3], cell algebra of
     * sampleRNN/lib/ops.py:505-553, gate order i|f|o|g): one packed matrix per layer, passed in Wg
     * ([K_l,4H], rows as above), bias in bg ([4H]), per-step inputs in seq_g ([T,B,4H]), gradient wrt the
     * pre-activations out in dG ([T,B,4H]); Wc / bc / seq_c / z / r / rh / c / dC are unused. */
    int cell;
    int seq_init;                     /* bit l set: seq_g[l]/seq_c[l] hold caller data (else scratch), see below */
    float* cst[PARROT_MAX_LAYERS];    /* [T+1,B,H] cell-state history (slot 0 = entering the window) */
    float* gate4[PARROT_MAX_LAYERS];  /* [T,B,4H] saved gate activations */
    float* dcell[PARROT_MAX_LAYERS];  /* [B,H] in: gradient wrt the final cell (0), out: wrt the initial cell */
    /* layer_norm = 1 (model.py:24-34, 703-722): the projections of the lower layers' outputs into layer l
     * (Fork h{j}_to_h{l}, index [l*PARROT_MAX_LAYERS + j], j < l) are normalised row-wise before they are
     * summed, so they cannot ride in the packed GEMM; the scan then runs on the chunked layer pipeline and
     * needs, per (l, j) pair and group: the Fork bias (ln_b*, taken out of bg/bc by the caller), a buffer for
     * the normalised projection (ln_y*, [T,B,width]; seq_bwd overwrites it with the gradient wrt the
     * PRE-norm projection, which the caller turns into the weight/bias gradients) and the row std (ln_s*,
     * [T,B]).  Rows of Wg/Wc keep the packed layout. */
    /* bf16 = 1 (BASELINE configs[3]): Wg_f / Wc_f / Wg_r / Wc_r are bf16 copies made by parrot_tile_weights_bf16
     * (mandatory then; H and E multiples of 32), the step GEMMs round the activations they read to bf16 and run on
     * v_mfma_f32_16x16x32_bf16 with f32 accumulation, the batched lower-layer projections of the chunked schedule take
     * the bf16 path of parrot_gemm.  States, gate activations, attention and all gradients buffers stay f32. */
    int layer_norm, bf16;
    const float* ln_bg[PARROT_MAX_LAYERS * PARROT_MAX_LAYERS];
    const float* ln_bc[PARROT_MAX_LAYERS * PARROT_MAX_LAYERS];
    float* ln_yg[PARROT_MAX_LAYERS * PARROT_MAX_LAYERS];
    float* ln_yc[PARROT_MAX_LAYERS * PARROT_MAX_LAYERS];
    float* ln_sg[PARROT_MAX_LAYERS * PARROT_MAX_LAYERS];
    float* ln_sc[PARROT_MAX_LAYERS * PARROT_MAX_LAYERS];
    /* Optional fragment-major copies of the packed layer matrices (parrot_tile_weights), same element count as
     * Wg[l] / Wc[l]: *_f for the forward products (mode 0; LSTM: lstm_H = H), *_r for the backward products
     * with the transpose (mode 1).  When all are given the scan reads the weights through them (contiguous
     * 1 KB wave loads); the caller refreshes them whenever the weights change.  NULL: plain matrices. */
    const float* Wg_f[PARROT_MAX_LAYERS];
    const float* Wc_f[PARROT_MAX_LAYERS];
    const float* Wg_r[PARROT_MAX_LAYERS];
    const float* Wc_r[PARROT_MAX_LAYERS];
    /* Optional [T,B,2] int32 scratch: per step and row the first / last context position whose window weight phi is
     * not exactly 0.0f (written by seq_fwd, read by seq_bwd).  Rows outside it are multiplied by exact zeros in
     * model.py:675-690 and its gradient, so the scan does not read them; NULL: all U rows are read.  An all-zero row saves
     * the empty support (U, -1); under PARROT_ATT_DENSE=1 every row saves the full range (0, U-1). */
    int* att_sup;
    /* Optional workspace of the persistent forward scan (PARROT_SCHEDULE=4): at least
     * parrot_decoder_persist_floats(desc) floats, ZERO-FILLED by the caller once.  It holds the machine's
     * fragment-major activation slabs, pre-activation buffers, unit table and barrier words.  With it (and GRU layers,
     * B <= 64, H and E multiples of 16, U <= 800, fragment-major weight copies present) seq_fwd runs the whole window as
     * one resident kernel: weights stationary in LDS, phases separated by grid barriers (parrot_amd/csrc/persist.h).
     * NULL, too small or a non-qualifying configuration: the launch schedules are used. */
    float* persist_ws;
    long long persist_ws_floats;
    /* Optional second accumulators of the backward scan (round 4; LSTM layers with bf16 operands): [T+1,B,H] per layer
     * for dh and dhup, [T+1,B,E] for dw and dw0, ZERO-FILLED by the caller once.  With all of them given the transposed
     * products of a backward tick (dP . W^T, K = 4H) are cut into two K halves handled by different workgroups -- a wide
     * workgroup's time is the time to stream its [B, K] operand -- and the second half's sums land here instead of in
     * dh / dhup / dw / dw0: stored into dh_b and dw0_b (one writer per slot), ADDED into dhup_b and dw_b (every layer above
     * adds its share: the caller zero-fills these two before every seq_bwd, as it does dhup and dw0); the state backward
     * and the attention backward of the next tick add both parts (so does the caller for slot 0).  NULL: one accumulator
     * per gradient, as before. */
    float* dh_b[PARROT_MAX_LAYERS];
    float* dhup_b[PARROT_MAX_LAYERS];
    float* dw_b;
    float* dw0_b;
    /* Third accumulators (same shapes and rules as dhup_b / dw_b / dw0_b; dw0_c is stored, the other two are added into
     * and zero-filled by the caller before every seq_bwd).  With all second AND third accumulators given, a 2-layer f32
     * GRU decoder runs the K-balanced backward tick (plans.hip bwd8): every K = 2H product of a tick is cut into its
     * update-gate and reset-gate halves writing separate buffers, layer 1 runs two ticks ahead of layer 0, and the
     * downward products of layer 1 ride in the NEXT tick's attention launch beside the attention backward blocks. */
    float* dhup_c[PARROT_MAX_LAYERS];
    float* dw_c;
    float* dw0_c;
    /* Optional (round 5; bf16 LSTM decoders whose backward tick is one launch): dG16[l], [T,B,4H] bf16 -- the backward scan
     * also leaves every pre-activation gradient row rounded to bf16 (nearest even: exactly what parrot_to_bf16 would make
     * of dG[l]), so the deferred weight-gradient products (parrot_gemm_bf16in) need no conversion pass over 3 x [T,B,4H]
     * floats.  parrot_decoder_writes_bf16_grads(plan) says whether the plan honours them (all given, fused backward). */
    void* dG16[PARROT_MAX_LAYERS];
} ParrotDecoderDesc;

/* Floats of persist_ws a plan for this descriptor needs; 0 when the configuration does not qualify for the persistent
 * scan (see above).  Only T, B, H, E, A, U, L, cell, layer_norm and the Wg_f / Wc_f pointers are read. */
long long parrot_decoder_persist_floats(const ParrotDecoderDesc* desc);
/* 1 when the plan's forward scan runs on the persistent phase machine. */
int parrot_decoder_is_persistent(void* plan);
/* The launch schedule the plan's scan runs on (PARROT_SCHEDULE, after the fall-backs for configurations a schedule does
 * not cover): 0 merged wavefront, 2 / 3 chunked pipelines, 5 balanced wavefront (attention beside the upper layers'
 * input projections), 6 two launches per tick (attention inside the gate launch). */
int parrot_decoder_schedule(void* plan);
/* Which backward tick the plan runs: 8 = the K-balanced tick with the downward products of the upper layers inside the
 * attention launch (GRU stacks of 2 or 3 layers, f32: reference depth model.py:312-347), 7 = the fused LSTM tick of
 * bf16-operand decoders, 0 = three launches per tick (attention + state backward, X, Y); schedule 3 runs the mirror of its
 * chunked forward pipeline and reports 0 whatever accumulators it is given. */
int parrot_decoder_backward_tick(void* plan);
/* Schedule tracing (test infrastructure of the library itself; runs without a GPU): instead of launching, the plan
 * records for every launch of direction `which` (0 forward, 1 backward) and every job in it the byte ranges of the
 * descriptor's buffers the job reads / writes.  Records are 5 x int64: launch index, job id (0..8 step-GEMM jobs, 100 the
 * attention (+ the state backward fused behind it), 200 + c state-backward chain c), kind (0 read, 1 write, 2 read +
 * write, 3 read behind an in-launch flag), lo, hi (byte addresses).  Returns the number of records (fills min(n, cap)
 * of them into `out`), or -(error code); launch schedules 0, 5 and 7 only.  PARROT_TRACE_ONLY=1 lets schedule 7 be
 * created on a box without a GPU. */
long long parrot_decoder_trace(void* plan, int which, long long* out, long long cap);
/* The same dry run, one record per job: 6 x int64 = launch index, job id, M (rows), N (output columns), K (sum over the
 * job's segments), epilogue code (SkEpi; -1 attention forward, -2 attention backward: then M, N, K = B, E, H).  What
 * tools/tick_model.py prices with the measured launch cost model. */
long long parrot_decoder_trace_jobs(void* plan, int which, long long* out, long long cap);
/* Waits for the device; 0, or non-zero when a persistent launch of this plan gave up (a workgroup waited ~1 s for a
 * rendezvous or for an operand that never arrived): the results of that window are invalid.  0 on the launch schedules. */
int parrot_decoder_status(void* plan);

int parrot_decoder_create(const ParrotDecoderDesc* desc, void** plan);
int parrot_decoder_writes_bf16_grads(void* plan);
int parrot_decoder_seq_fwd(void* plan, void* stream);
int parrot_decoder_seq_bwd(void* plan, void* stream);
int parrot_decoder_destroy(void* plan);

/* ------------------------------------------------------------------------------------------
 * Training: readout stack and output layer composed (model.py:739-755 with the MSE head and no layer norm).
 *   readouts = sum_s x_s . Wr_s + sum_i rb_i,   pred = readouts . Wo + bo
 * has nothing non-linear in between, so pred = sum_s x_s . W'_s + b' with W' = Wr . Wo [sum K_s, O] and
 * b' = (sum_i rb_i) . Wo + bo: products of width O <= 64 instead of R.  parrot_readout_composed_fwd composes W' and b'
 * from the current weights (accumulated in double, rounded once) and writes pred; parrot_readout_composed_bwd takes
 * dp = d cost / d pred and, by the chain rule through the same composition,
 *   dx_s = dp . W'_s^T                                   stored below zero_rows zero-filled rows (slot 0 of a history),
 *   gWr += dW' . Wo^T,  gWo += Wr^T . dW' + rbsum^T (x) sum_m dp,   with dW' = sum_m x[m,:]^T dp[m,:],
 *   grb_i += (sum_m dp) . Wo^T,  gbo += sum_m dp.
 * Segments: x_s [M, K_s] row-major, leading dimension ldx[s] (a multiple of 4, 16-byte aligned base), K_s a multiple
 * of 16; Wr [sum K_s, R] holds the segments' rows in order.  The backward call reads the W' its forward call left in
 * the workspace: call them in pairs, weights unchanged in between.  The reduction over M is cut into slices of
 * slice_rows rows (0: chosen by the library) whose partial tiles are added in slice order: no float atomics, results
 * are bit-reproducible.  The workspace is the caller's: parrot_readout_composed_ws_floats(desc) floats, 16-byte
 * aligned, its size in ws_floats; the calls neither allocate nor synchronise.
 * ------------------------------------------------------------------------------------------ */
#define PARROT_READOUT_MAX_SEG 4
typedef struct ParrotReadoutComposedDesc {
    long long M;                  /* rows (T * B) */
    long long ws_floats;          /* floats behind the workspace pointer handed to the calls */
    int nseg, R, O, zero_rows;    /* segments, readout width, output width (<= 64), rows zero-filled on top of each dx_s */
    int slice_rows, nbias;        /* rows of M per slice of the dW' reduction (0: automatic); readout bias vectors */
    int K[PARROT_READOUT_MAX_SEG];
    int ldx[PARROT_READOUT_MAX_SEG];
    int lddx[PARROT_READOUT_MAX_SEG];
    int ldwr, ldwo, ldp, lddp;    /* leading dimensions of Wr (>= R), Wo (>= O), pred (>= O), dp (>= O) */
    int ldgwr, ldgwo;             /* leading dimensions of gWr (>= R) and gWo (>= O) */
    const float* x[PARROT_READOUT_MAX_SEG];
    const float* Wr; const float* Wo;
    const float* rb[PARROT_READOUT_MAX_SEG];   /* [R] each: the *_to_readout biases */
    const float* bo;              /* [O] */
    float* pred;                  /* [M, O]  forward out */
    const float* dp;              /* [M, O]  backward in */
    float* dx[PARROT_READOUT_MAX_SEG];  /* [zero_rows + M, K_s], leading dimension lddx[s]: rows < zero_rows = 0, then dp . W'_s^T */
    float* gWr; float* gWo;       /* [sum K_s, R], [R, O]   accumulated into */
    float* grb[PARROT_READOUT_MAX_SEG]; /* [R] each           accumulated into */
    float* gbo;                   /* [O]                    accumulated into */
} ParrotReadoutComposedDesc;

/* Floats of workspace the two calls need for this descriptor (sizes only are read), or -PARROT_ERR_BADARG. */
long long parrot_readout_composed_ws_floats(const ParrotReadoutComposedDesc* desc);
int parrot_readout_composed_fwd(const ParrotReadoutComposedDesc* desc, float* ws, void* stream);
int parrot_readout_composed_bwd(const ParrotReadoutComposedDesc* desc, float* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Autoregressive decode: the theano.scan over `sample_step` of Parrot.sample_model_fun
 * (model.py:882-1057) for the MSE ("greedy") head: x_t = readout_to_output(readouts_t), or the GMM
 * head (gmm_K > 0 below): x_t sampled from the mixture the readout parameterises.
 * Same packed weights as above plus, per layer, the fed-back-output rows (out_to_h*, present
 * when weak/full feedback is on; Wfg[l] [O,2H], Wfc[l] [O,H], NULL otherwise), and the readout
 * stack Wr = [h1_to_readout ; .. ; hL_to_readout ; att_to_readout] [L*H+E, R], br = summed bias,
 * Wo [R,O], bo [O].  x is stored with leading dimension ldx >= O (padded rows are zero).
 * Whole sequences are captured into one hipGraph when use_graph = 1.
 * ------------------------------------------------------------------------------------------ */
typedef struct ParrotSampleDesc {
    int S, B, H, E, A, U, L, O, R, ldx, att_type, use_graph;
    float eps, alignment, sharpening, timing;
    const float* Wg[PARROT_MAX_LAYERS];
    const float* Wc[PARROT_MAX_LAYERS];
    const float* bg[PARROT_MAX_LAYERS];
    const float* bc[PARROT_MAX_LAYERS];
    const float* Wfg[PARROT_MAX_LAYERS];
    const float* Wfc[PARROT_MAX_LAYERS];
    const float* seq_c[PARROT_MAX_LAYERS]; /* [B,H]  constant additive inputs (speaker) or NULL */
    const float* seq_g[PARROT_MAX_LAYERS]; /* [B,2H] */
    const float* WattT; const float* batt;
    const float* Wr; const float* br;      /* [L*H+E, R], [R] (+ speaker readout folded in by caller) */
    const float* radd;                     /* [B,R] constant additive readout term or NULL */
    const float* Wo; const float* bo;      /* [R,O], [O] */
    const float* oadd;                     /* [B,O] constant additive output term or NULL */
    const float* ctx;                      /* [B,U,E] */
    float* x;      /* [S+1,B,ldx] slot 0 = initial_x (zeros, model.py:834-835) */
    float* h[PARROT_MAX_LAYERS]; /* [2,B,H] ping-pong, slot 0 = initial state */
    float* w;      /* [S+1,B,E]  */
    float* kappa;  /* [S+1,B,A]  */
    float* a;      /* [S,B,A] (pi_att) */
    float* bwork;  /* [B,A] scratch */
    float* phi;    /* [S,B,U] */
    float* zwork; float* rwork; float* rhwork; float* readout; /* [B,H],[B,H],[B,H],[B,R] scratch */
    /* GMM head (which_cost = 'GMM', model.py:1017-1033 + sample_gmm :94-118); gmm_K = 0 selects the MSE head.
     * Randomness is supplied by the caller: unif [S,B] in [0,1) picks the component exactly like Theano's
     * multinomial (first k with cumsum(pi) > u), noise [S,B,O] ~ N(0,1) scales sigma. */
    int gmm_K, reserved2;
    float sampling_bias, reserved3;
    const float* Wmu; const float* bmu; const float* Wsig; const float* bsig; const float* Wco; const float* bco;
                                 /* [R,O*K],[O*K] x2 (column o*K + k), [R,K],[K] */
    const float* add_mu; const float* add_sig; const float* add_co; /* [B,O*K] x2, [B,K] speaker terms or NULL */
    const float* unif; const float* noise;
    float* gmm_mu; float* gmm_sig; float* gmm_co;   /* scratch [B,O*K] x2, [B,K] */
    float* pi_out;                                   /* [S,B,K] mixture weights per step (the reference's `pi`) */
    /* LSTM variant (cell = 1): Wg/bg/Wfg/seq_g are 4H wide, Wc/bc/Wfc/seq_c unused; cwork [2,B,H] ping-pong
     * cell state (slot 0 = initial cell), gwork [B,4H] scratch. */
    int cell, reserved5;
    float* cwork[PARROT_MAX_LAYERS];
    float* gwork;
    /* layer_norm = 1 (model.py:899-1006 with _apply_norm active): the feedback Fork out_to_h{l}, the Forks
     * h{j}_to_h{l} and the h{l}_to_readout projections are taken as separate small GEMMs, normalised row-wise
     * and summed; their biases therefore come separately (bfg/bfc, ln_bg/ln_bc [l*PARROT_MAX_LAYERS + j],
     * br_l) and must NOT be folded into bg/bc/br.  seq_g/seq_c hold the already normalised speaker terms.
     * ln_scratch: at least B * (5*Ng + 5*Nc + (L+1)*R) floats (Ng/Nc = widths of the two groups). */
    int layer_norm, reserved7;
    const float* bfg[PARROT_MAX_LAYERS];
    const float* bfc[PARROT_MAX_LAYERS];
    const float* ln_bg[PARROT_MAX_LAYERS * PARROT_MAX_LAYERS];
    const float* ln_bc[PARROT_MAX_LAYERS * PARROT_MAX_LAYERS];
    const float* br_l[PARROT_MAX_LAYERS];
    float* ln_scratch;
    long long ln_scratch_floats;
    /* Optional: decode on the persistent phase machine (parrot_amd/csrc/persist.h) -- the whole S-step loop as one
     * resident kernel, 2L + 3 barrier-separated phases per step instead of 2L + 3 launches.  MSE head (a GMM head:
     * Wrh_t / rh_const at the end of this struct), no layer_norm, B <= 64, O <= 64 <= ldx.  The caller provides fragment-major copies (parrot_tile_weights, mode 0) of
     *   Wg_t[l] / Wc_t[l]: [K_l + F_l, 2H] / [K_l + F_l, H] = the packed layer matrix with the feedback rows Wfg / Wfc
     *                      appended and zero-padded to F_l = 64 rows (F_l = 0 without feedback into the layer),
     *   Wr_t: [L*H + E, R],   Wo_t: [R, 64] (columns >= O zero),
     * bo_pad [64] (zeros beyond O), oadd_pad [B, 64] when oadd is used, and a ZERO-FILLED workspace of
     * parrot_sample_persist_floats(desc) floats.  Anything missing or non-qualifying: the per-step launches run.
     * The h ping-pong buffers keep the initial state (slot 0) only; PARROT_SAMPLE_PERSIST=0 disables the machine.
     * LSTM layers (cell = 1): Wg_t[l] is [K_l + F_l, 4H] = the packed 4H-wide layer matrix with the feedback rows Wfg
     * appended (zero-padded to F_l = 64), fragment-major with gate-interleaved columns = parrot_tile_weights(.., mode 0,
     * lstm_H = H); Wc_t is ignored; bg / seq_g stay in their natural [i | f | o | g] order.  Wro_t and ro_const (below) are
     * required: a step is L + 2 whole-K phases (layer 0, attention, layers 1 .. L-1, composed output); Wr_t / Wo_t /
     * bo_pad / oadd_pad / Wgx_t / Wcx_t / Watt_t are not used.  The machine reads slot 0 of h[l] and cwork[l] (initial state
     * and cell) and leaves both ping-pong buffers as they were; states and cells of the loop live in the workspace. */
    const float* Wg_t[PARROT_MAX_LAYERS];
    const float* Wc_t[PARROT_MAX_LAYERS];
    const float* Wr_t; const float* Wo_t; const float* bo_pad; const float* oadd_pad;
    float* persist_ws;
    long long persist_ws_floats;
    /* Optional (round 4): with the MSE head and no layer norm, readout -> output is linear in the readout's operands
     * (model.py:992-1013).  Given
     *   Wro_t:    fragment-major copy of Wr . Wo, [L*H + E, 64] (columns >= O zero), and
     *   ro_const: [B, 64] row-major = (br + radd) . Wo + bo + oadd (columns >= O zero),
     * the machine computes x[t+1] straight from [h_0 .. h_{L-1} ; w] in ONE phase and cuts every product of the step
     * along K by the age of its operands (2L + 2 phases per step, each walking only the rows of its newest operand;
     * plans.hip, build_persist_pieces).  NULL, or PARROT_PM_PIECES=0: the 2L + 3 whole-K phases above. */
    const float* Wro_t;
    const float* ro_const;
    /* Optional (round 5), on top of Wro_t / ro_const: the fed-back frame out of the step's dependency chain.  With feedback
     * into layer 0 only (weak feedback, model.py:899-911) and L >= 2, x[t+1] = x_pre + h_{L-1}[t+1] . A with
     * A = Wro[(L-1)H : L H] and x_pre (the other rows' shares plus ro_const) known two phases before h_{L-1}, so layer 0's
     * next gates take  x_pre . Wfg  (K = 64, early)  +  h_{L-1} . (A . Wfg)  (K = H, the critical piece) and the output
     * product leaves the chain: 2L + 1 phases per step.  Given, for l = 0, fragment-major copies of
     *   Wgx_t[0] / Wcx_t[0]: [H + E + 64 + H, 2H] / [.., H] = the rows of Wg_t[0] / Wc_t[0] followed by A . Wfg / A . Wfc
     *                        (composed in double precision, rounded once; Wf zero-padded to 64 rows)
     * the machine plans that way; NULL, other feedback patterns, L = 1 or PARROT_PM_FBC=0: the 2L + 2 phases above. */
    const float* Wgx_t[PARROT_MAX_LAYERS];
    const float* Wcx_t[PARROT_MAX_LAYERS];
    /* Optional (round 5, B <= 16, 3A <= 32): Watt_t = fragment-major copy (parrot_tile_weights, mode 0) of the attention
     * projection as an [H, 32] matrix (column j < 3A = row j of WattT, the rest zero).  Layer 0's candidate units then also
     * multiply the h_1 tile they have just computed by their 16 rows of it and publish [B, 32] partial sums; the attention
     * row adds H / 16 of them instead of reading its state row and the whole projection matrix (model.py:926-930 is the
     * same sum, associated tile by tile).  NULL or PARROT_PM_ATTFOLD=0: the row computes the projection itself. */
    const float* Watt_t;
    /* bf16 = 1: decode with bf16 operands.  The one product per layer and step, [h_l[t] ; w ; h_0[t+1] .. h_{l-1}[t+1] ; x[t]]
     * . Wg_t[l], rounds BOTH operands to bf16 (nearest even) where they enter the product and accumulates in f32; states,
     * cells, biases, additive inputs, the attention and the composed output product stay f32.  LSTM stacks on the
     * persistent machine only: cell = 1, MSE head (never a GMM head), no layer_norm, B <= 64, H and E multiples of 32, workspace given, and
     *   Wg_t16[l]: the matrix of Wg_t[l] (feedback rows appended, padded to 64) as parrot_tile_weights_bf16(.., mode 2,
     *              lstm_H = H), rows*cols bf16; Wg_t[l] is then not read and may be NULL.
     * Resident bf16 slabs take half the LDS, so more of them stay on chip, and the streamed ones move half the bytes.
     * There is no f32 decode behind this switch: parrot_sample_create returns PARROT_ERR_UNSUPPORTED for every configuration
     * the bf16 machine does not take (parrot_sample_persist_floats returns 0 for them).
     * GRU stacks (cell = 0), opt-in (PARROT_PM_GRU_BF16=1; unset or 0: refused as before): the two products per layer and step,
     * gates [h_l[t] ; ..] . Wg_t[l] and candidate [r * h_l[t] ; ..] . Wc_t[l], round both operands the same way (r * h_l[t] is
     * rounded where it enters the candidate product); gate activations, the state blend, the attention and the readout /
     * output tiles stay f32.  Same conditions (MSE head, no layer_norm, B <= 64, H and E multiples of 32), and
     *   Wg_t16[l] / Wc_t16[l] (the last field of this struct): the matrices of Wg_t[l] (2H columns) / Wc_t[l] (H columns),
     *              feedback rows appended and padded to 64, as parrot_tile_weights_bf16(.., mode 2, lstm_H = 0); Wg_t[l] and
     *              Wc_t[l] are then not read and may be NULL.
     * Both GRU programs take them (the step cut along K, or the whole-K phases under PARROT_PM_PIECES=0 / without Wro_t);
     * Wgx_t / Wcx_t / Watt_t are NOT taken under bf16: the composed rows A . Wf and the folded projection would round at other
     * points than x . Wf and h . Watt do.  The output tiles (Wro_t, or Wr_t / Wo_t) are f32 units of the same program. */
    int bf16, reserved8;
    const void* Wg_t16[PARROT_MAX_LAYERS];
    /* eou_extra > 0: stop at the end of the utterance, inside the persistent machine.  Row b's predicate at step t (0-based)
     * is  phi[t, b, eou_pos[b]] > phi[t, b, j] for all j < eou_ncmp[b]  on the f32 values stored to phi (strict; a NaN
     * never holds; eou_ncmp[b] = 0 holds at once).  eou_first[b] (output, [B] ints) = the first step at which it held, or
     * -1; the row's length is min(S, eou_first[b] + eou_extra), S for a row that never fires.  Once every row has fired the
     * run ends after frame T_stop = the longest row: every output row below T_stop is bit-identical to a run without the
     * stop, later rows are unspecified (parrot_sample_steps_run reports T_stop).  eou_pos, eou_ncmp, eou_first: device
     * arrays of B ints, 0 <= eou_pos[b] < U, 0 <= eou_ncmp[b] <= U (clamped); eou_extra >= 8.  The stop exists on the
     * persistent machine only: parrot_sample_create returns PARROT_ERR_UNSUPPORTED for a descriptor that asks for it and
     * gets no machine plan (GMM head without PARROT_PM_GMM=1, layer_norm, B > 64, PARROT_SAMPLE_PERSIST=0, no workspace, eou_extra < 8, an array
     * missing); the per-step launches are never substituted.  0: every run decodes all S steps. */
    const int* eou_pos;
    const int* eou_ncmp;
    int* eou_first;
    int eou_extra, reserved9;
    /* Optional, opt-in (PARROT_PM_GMM=1; unset or 0: a GMM head decodes as per-step launches whatever is given here): the GMM
     * head on the persistent machine.  Without layer_norm nothing non-linear sits between the readout stack and the three
     * head projections, so with Wh = [Wmu | Wsig | Wco] ([R, 2 O K + K] in that column order, zero-padded to rh_cols =
     * a multiple of 16 columns) the caller hands over
     *   Wrh_t:    fragment-major copy (parrot_tile_weights, mode 0) of Wr . Wh, [L*H + E, rh_cols], composed in double
     *             precision and rounded once,
     *   rh_const: [B, rh_cols] row-major = (br + radd) . Wh + [bmu | bsig | bco] + [add_mu | add_sig | add_co].
     * A step then ends in a head phase (rh_cols / 16 column tiles of [h_0 .. h_{L-1} ; w] . Wrh_t + rh_const, kept as a
     * write-once history [S, B, rh_cols] in the workspace) and a sampling phase (one unit per batch row: mixture weights,
     * the pick against unif, x[t+1] = mu + (exp(sig_hat - sampling_bias) + eps) * noise, pi_out) in place of the readout
     * and output phases: GRU stacks 2L + 3 whole-K phases, LSTM stacks L + 3; parrot_sample_is_persistent reports 1.
     * Needs gmm_K <= 64, unif, noise and pi_out, f32 operands (bf16 = 0), rh_cols / 16 tiles within the machine's
     * workgroups (x 2 where an LSTM layer has more tiles than workgroups), and everything the machine needs of an MSE
     * head except Wr_t / Wo_t / bo_pad / oadd_pad / Wro_t / ro_const / Wgx_t / Wcx_t / Watt_t, which are not read.
     * gmm_mu / gmm_sig / gmm_co stay untouched on the machine.  The end-of-utterance stop (eou_*) applies as it is. */
    const float* Wrh_t;
    const float* rh_const;
    int rh_cols, reserved10;
    /* bf16 = 1, GRU stacks (PARROT_PM_GRU_BF16=1): the bf16 copies of the candidate matrices, see Wg_t16 above.  Appended
     * here: the fields above keep their offsets. */
    const void* Wc_t16[PARROT_MAX_LAYERS];
} ParrotSampleDesc;

long long parrot_sample_persist_floats(const ParrotSampleDesc* desc);
/* 0: per-step launches; 1: the machine with whole-K phases (GRU: 2L + 3; LSTM: L + 2, L + 3 with a GMM head); 2: the machine with the step cut
 * along K (GRU, Wro_t given); 3: the same with the fed-back frame out of the chain (Wgx_t / Wcx_t given, 2L + 1 phases) */
int parrot_sample_is_persistent(void* plan);
/* 1: the plan runs the machine with bf16 operands (ParrotSampleDesc::bf16); 0: every product has f32 operands */
int parrot_sample_is_bf16(void* plan);
/* Plans the decode machine for `desc` with `nwg` workgroups WITHOUT touching device memory (pointers are only used for
 * address arithmetic) and replays the unit table symbolically: every read must find its value written in an earlier
 * phase, every buffer element is written once.  info16: [0] phases per step, [1] partial-sum buffers, [2] checker
 * verdict (0 ok), [3] units per step, [4 + s] units in phase s, [14] units that stream their weights, [15] bit 0: the
 * fed-back frame is out of the chain (Wgx_t / Wcx_t), bit 1: the attention projection is folded into the candidate units (Watt_t).
 * 0, or PARROT_ERR_UNSUPPORTED when the configuration does not take this plan.  Used by the CPU tests. */
int parrot_sample_plan_pieces_dry(const ParrotSampleDesc* desc, int nwg, int* info16);
/* The same dry run, reduced to one number: the FNV-1a 64-bit hash of the placed unit table, of the program's attention,
 * sampling, init and fill records, and of T, ticks, phases, units per workgroup and workgroups.  The dry run carves a
 * workspace at a fixed fake address, so equal descriptors (pointers included) and switches give equal digests, in any
 * process.  Same return codes; *digest = 0 when there is no plan.  Used by the CPU tests to hold the planners still. */
int parrot_sample_plan_digest_dry(const ParrotSampleDesc* desc, int nwg, unsigned long long* digest);
/* Like parrot_decoder_status, for a decode plan. */
int parrot_sample_status(void* plan);
/* 1: the plan stops at the end of the utterance (ParrotSampleDesc::eou_extra > 0 on the machine); 0: it runs all S steps */
int parrot_sample_stops_early(void* plan);
/* Frames the last parrot_sample_run completed (synchronises like parrot_sample_status): T_stop <= S for a plan that stops
 * early, S for every other plan. */
int parrot_sample_steps_run(void* plan, int* steps);

/* Per-row decode controls: row b of every later run decodes with timing[b] / sharpening[b] / sampling_bias[b] in place of
 * ParrotSampleDesc::timing / sharpening / sampling_bias -- b = exp(b_hat) * sharpening[b] + eps, kappa = kappa_prev +
 * alignment * exp(k_hat) / timing[b], exp(sig_hat - bias[b]) + eps, co_hat * (1 + bias[b]) -- on whichever path the plan
 * decodes (the persistent machine or the per-step launches), with the end-of-utterance stop as without it.  Each argument
 * is a device array of B floats, or NULL: that control stays the descriptor's scalar for every row.  The caller owns the
 * arrays, keeps them alive as long as the plan, and rewrites their CONTENTS between runs as it likes; the values must be
 * finite, timing and sharpening > 0 (not checked).  All three NULL: no controls, the plan is what parrot_sample_create
 * made.  Call it before the plan's first parrot_sample_run: afterwards it returns PARROT_ERR_BADARG (a captured graph
 * holds the pointers by value).  sampling_bias != NULL on a plan without a GMM head (gmm_K = 0): PARROT_ERR_BADARG.
 * Equal values give equal bits: row b decodes exactly as it does under a descriptor that carries its three values. */
int parrot_sample_set_row_controls(void* plan, const float* timing, const float* sharpening, const float* sampling_bias);

int parrot_sample_create(const ParrotSampleDesc* desc, void** plan);
int parrot_sample_run(void* plan, void* stream);
int parrot_sample_destroy(void* plan);

/* Forced frames (priming), per row: a decode descriptor with three fields behind it.  While t < n_forced[b] the frame fed
 * back into step t + 1 of row b is forced[t, b] instead of the model's own -- x[t + 1, b] = forced[t, b]; an MSE head's
 * output frame is replaced, a GMM head's draw.  From step n_forced[b] on the row decodes as ever, from the state (layers,
 * kappa, w) the prompt left.  Rows are independent; n_forced[b] = 0 is a free row.
 *   base:     the decode descriptor, every field as above (its offsets are ParrotSampleDesc's: base is the first member).
 *   forced:   [S, B, ldx] f32, device.  Columns >= O are not read: they are fed back, and written to x, as zero.
 *   n_forced: [B] int32, device, 0 <= n_forced[b] <= S (not checked).
 *   own_x:    [S, B, ldx] f32, device, output: what the model computed (MSE) or drew (GMM) at step t BEFORE the select;
 *             equal to x[t + 1] wherever the row is not forced.
 * The three fields follow the END of ParrotSampleDesc in a type of their own, not inside it: the library copies a descriptor
 * by value, so a ParrotSampleDesc that grew would make it read past the buffer of every caller built against this header
 * as it was, and parrot_sample_create keeps taking exactly the bytes it took.
 * All three NULL: no forcing, the plan is parrot_sample_create(&base)'s; otherwise all three must be given
 * (PARROT_ERR_BADARG).  Forcing is a property of the plan: a forced plan cannot take the fed-back frame out of the step's
 * chain (x[t + 1] = x_pre + h_{L-1} . A does not hold on a forced step), so Wgx_t / Wcx_t are not taken and a GRU stack with
 * an MSE head decodes on the 2L + 2 phases that PARROT_PM_FBC=0 gives; the attention fold (Watt_t) does not depend on the
 * composed path and stays.  The pointers are held by value (a captured graph replays with them); their CONTENTS may be
 * rewritten between runs.  Every path takes them: the persistent machine (GRU and LSTM programs, MSE and GMM heads, the
 * end-of-utterance stop, the row controls) and the per-step launches.  base.bf16 = 1 with forcing: PARROT_ERR_UNSUPPORTED. */
typedef struct ParrotSampleForcedDesc {
    ParrotSampleDesc base;
    const float* forced;
    const int* n_forced;
    float* own_x;
} ParrotSampleForcedDesc;
/* parrot_sample_create / parrot_sample_persist_floats / the two dry entries below, for a descriptor with forced frames: the
 * plan, the workspace size, info16 and the digest of the FORCED plan (info16[15] bit 0 is clear: no composition).  The
 * plan is run, queried and destroyed like any other (parrot_sample_run, _status, _steps_run, _set_row_controls, _destroy). */
int parrot_sample_create_forced(const ParrotSampleForcedDesc* desc, void** plan);
long long parrot_sample_persist_floats_forced(const ParrotSampleForcedDesc* desc);
int parrot_sample_plan_pieces_dry_forced(const ParrotSampleForcedDesc* desc, int nwg, int* info16);
int parrot_sample_plan_digest_dry_forced(const ParrotSampleForcedDesc* desc, int nwg, unsigned long long* digest);

/* Decode state: resumable decode calls.  A state is one packed device buffer [B, W] of f32, row-major; row b holds what
 * utterance b carries from frame t to frame t + 1,
 *   [ x (ldx) | kappa (A) | w (E) | h_0 (H) .. h_{L-1} (H) | c_0 .. c_{L-1} (H each, cell = 1 only) ],
 * so admitting or evicting an utterance is a row copy.  States are f32 on every plan (bf16 operands included).
 * parrot_sample_state_floats: W = ldx + A + E + L H (1 + cell); it reads the descriptor's integers only and touches no
 *   device (0 for a NULL descriptor).
 * parrot_sample_load_state: scatters `state` into the slots the next parrot_sample_run enters through -- slot 0 of x, kappa,
 *   w, h[l] and cwork[l] -- on the stream; the run then decodes frames t .. t + S - 1 of every row exactly as a longer
 *   call would have, provided the plan keeps the fed-back frame on the step's chain (no Wgx_t / Wcx_t: with them the first
 *   step of a call rounds x[0] . Wf differently from a step inside one, and a cut shows in the last bits).
 * parrot_sample_save_state: gathers the state after frame S of the plan's last run -- x[S], kappa[S], w[S]; the layers'
 *   states and cells from row S of the machine's histories, on the per-step launches from the ping-pong slot the run ended
 *   on -- into `state`, on the stream.  After a parrot_sample_load_state that no run has followed it returns the loaded
 *   state.  PARROT_ERR_UNSUPPORTED on a plan that stops early (eou_extra > 0: frame S need not exist); PARROT_ERR_BADARG on
 *   a plan that has neither run nor been loaded.
 * Both work on every plan parrot_sample_create and parrot_sample_create_forced make, and return PARROT_ERR_BADARG on a
 * NULL argument.  Without a load a run enters through whatever the caller wrote into the same slots, as it always has. */
long long parrot_sample_state_floats(const ParrotSampleDesc* desc);
int parrot_sample_save_state(void* plan, float* state, void* stream);
int parrot_sample_load_state(void* plan, const float* state, void* stream);

int parrot_plan_last_error(void* plan);

/* ------------------------------------------------------------------------------------------
 * Optimiser step next to the path (train.py:100-108): StepClipping(threshold) o Adam on the flat
 * parameter buffer.  gnorm_sq is a device scalar filled by parrot_sumsq (after the gradient
 * all-reduce in data-parallel runs); grad_scale rescales the raw gradient first (1/world_size).
 * ------------------------------------------------------------------------------------------ */
int parrot_sumsq(const float* x, size_t n, float* out, void* stream);

/* Fragment-major copy of a row-major weight matrix W [rows, cols] (leading dimension ld; rows, cols multiples
 * of 16) for the recurrent-step kernel: 256-float blocks ordered [column tile][16-deep chunk], each holding the
 * 64 lanes' MFMA operand quads.  mode 0: for products x . W (tiles over columns, chunks over rows; lstm_H > 0
 * applies the gate-interleaved column order of the fused LSTM step, cols = 4*lstm_H); mode 1: for products
 * x . W^T (tiles over rows, chunks over columns).  out: rows*cols floats. */
int parrot_tile_weights(const float* W, int rows, int cols, int ld, float* out, int mode, int lstm_H, void* stream);
/* The same copy rounded to bf16 (round to nearest even) for the bf16 operand mode of the decoder scan
 * (ParrotDecoderDesc::bf16): 1 KB blocks of 16 columns x 32 K-rows in v_mfma_f32_16x16x32_bf16 operand order.  The
 * K extent (rows in mode 0, cols in mode 1) must be a multiple of 32, the other one of 16.  out: rows*cols bf16.
 * mode 2: for the bf16 decode machine (ParrotSampleDesc::bf16).  Tiles, chunks and columns as mode 0 (lstm_H applies), but
 * the eight K rows of lane (kk, i) of chunk c are 32c + 4kk .. + 3 and 32c + 16 + 4kk .. + 3 -- the rows the same lane of
 * two consecutive f32 fragment-major activation blocks holds, so the machine rounds its activations in place and moves
 * nothing between lanes (an MFMA is indifferent to a permutation of K that both operands share). */
int parrot_tile_weights_bf16(const float* W, int rows, int cols, int ld, void* out, int mode, int lstm_H, void* stream);

/* _simple_norm / _apply_norm of the reference (model.py:24-34; used when layer_norm=True on the Fork outputs
 * and readout projections, model.py:585-620, 703-722, 746): y = (x - mean) / (eps + std) over the last axis
 * (population std, no affine).  x [R,N] (leading dimension ldx); y [R,N] may alias x; sigma [R] receives the
 * row std (saved for the backward); add_dst (or NULL) [R,N] gets += y. */
int parrot_simple_norm_fwd(const float* x, int ldx, float* y, int ldy, float* sigma, long long R, int N, float eps,
                           float* add_dst, int ld_add, void* stream);
/* Backward of the above: dx [R,N] (may alias dy or y) = J^T dy, from the saved y and sigma. */
int parrot_simple_norm_bwd(const float* dy, int lddy, const float* y, int ldy, const float* sigma, float* dx,
                           int lddx, long long R, int N, float eps, int accumulate, void* stream);
int parrot_adam_clip_step(float* param, const float* grad, float* m, float* v, size_t n,
                          const float* gnorm_sq, float grad_scale, float clip_threshold, float lr,
                          float beta1, float beta2, float eps, int step, void* stream);

/* ------------------------------------------------------------------------------------------
 * Audio quantisers (quantize.py:14-99).  x is [rows, n] float32; every row is min-max normalised
 * in float64 exactly as quantize.__batch_quantize does.  mode 0: mu-law -> int16 out,
 * mode 1: linear(q_levels) -> int32 out.  ws = device scratch of 2*rows doubles.
 * parrot_mu2linear: int32 class indices -> float32 amplitudes (quantize.py:68-78).
 * ------------------------------------------------------------------------------------------ */
int parrot_batch_quantize(const float* x, int rows, int n, int ld, double* ws, void* out, int ldo, int mode,
                          int q_levels, void* stream);
int parrot_mu2linear(const int32_t* q, size_t n, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-side operators of the SampleRNN sample-level tier (round 5; parrot_amd/csrc/trainops.hip).
 *
 * Embedding (sampleRNN/lib/ops.py:252-266) followed by SampleLevel.L1_PrevSamples (three_tier.py:486-497: a
 * [FS*EMB, DIM] Linear without bias over the FS concatenated embeddings) as a gather-sum over the folded table
 * tbl[j][q][:] = Embedding[q] . W1[j*EMB:(j+1)*EMB, :] (the form the generation loop uses, SampleRnnGenDesc::emb_tbl):
 *   parrot_gather_sum_fwd:  y[i,:] = add[i,:] + sum_{j<J} tbl[j][idx[i*J + j]][:]     (add may be NULL; summed in j order)
 *   parrot_gather_sum_bwd:  dtbl[j][q][:] (+)= sum over the rows i with idx[i*J + j] == q of dy[i,:]
 * The backward is a SEGMENTED sum, no scatter-add: perm [J,N] lists, per j, the rows sorted by (idx[.,j], row) (a stable
 * sort, so the order of the addends depends on the indices only) and offs [J,Q+1] the first position of every bin in that
 * order (offs[j][Q] = N).  ws: parrot_gather_sum_bwd_ws_floats(N,J,Q,D) floats of scratch.  D % 4 == 0, 16-byte aligned.
 * N == 0: the forward returns 0 and writes nothing; the backward returns PARROT_ERR_BADARG (there are no bins to sum:
 * it neither zeroes dtbl nor launches anything).
 *
 * Softmax cross-entropy with integer targets (three_tier.py:565-584, T.nnet.categorical_crossentropy(softmax(.), target)):
 *   parrot_softmax_ce_fwd:  lse[i] = log sum_q exp(logits[i,q]),  ce[i] = lse[i] - logits[i, target[i]]
 *   parrot_softmax_ce_bwd:  dlogits[i,q] = rowscale[i] * (exp(logits[i,q] - lse[i]) - [q == target[i]])
 * parrot_relu_gate: out = dy where gate > 0, else 0 (n % 4 == 0; ReLU backward where no product can carry it).
 * ------------------------------------------------------------------------------------------ */
int parrot_gather_sum_fwd(const float* tbl, const int* idx, const float* add, int ldadd, float* y, int ldy, long long N,
                          int J, int Q, int D, void* stream);
long long parrot_gather_sum_bwd_ws_floats(long long N, int J, int Q, int D);
int parrot_gather_sum_bwd(const float* dy, int lddy, const int* perm, const int* offs, float* dtbl, float* ws,
                          long long ws_floats, long long N, int J, int Q, int D, int accumulate, void* stream);
int parrot_softmax_ce_fwd(const float* logits, int ld, const int* target, long long rows, int Q, float* lse, float* ce,
                          void* stream);
int parrot_softmax_ce_bwd(const float* logits, int ld, const int* target, const float* lse, const float* rowscale,
                          long long rows, int Q, float* dlogits, int ldd, void* stream);
int parrot_relu_gate(const float* dy, const float* gate, float* out, long long n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Label tables of the text encoder (parrot_amd/csrc/labeltables.hip).  The encoder's input rows are rows of the
 * LookupTable (model.py:233-238): x = embed_label.W[labels], Q distinct rows.  So the Fork products x . W + b
 * (model.py:226-231) are rows of P = embed_label.W . W + b [Q, cols], and their Theano gradient needs only
 * S[q] = sum over the rows with label q of dY[row]:  dW = embed_label.W^T . S,  db = sum_q S[q],
 * d embed_label.W = S . W^T.  Up to four matrices (candidate / gate inputs of both directions) per call.
 *   parrot_label_gather:  rows[s][i,:] = tbl[s][labels[i],:]
 *   parrot_label_segsum:  sums[s][q,:] = sum over the i with labels[i] == q of rows[s][i,:]  (overwritten; a label that
 *                         never occurs gives a zero row).  Fixed summation order, no float atomics: same bits every
 *                         run; accumulated in double and rounded once.
 * labels [N] int32 in [0, Q) (values outside are clamped into the table, never read past it), D[s] % 4 == 0, 16-byte
 * aligned matrices, Q <= 64 (parrot_label_tables_supported).  ws: parrot_label_segsum_ws_floats(N, Q, sum of D) floats, 8-byte aligned.
 * ------------------------------------------------------------------------------------------ */
typedef struct ParrotLabelTablesDesc {
    long long N;              /* rows */
    int Q, nseg;              /* table rows; matrices in this call (1..4) */
    const int* labels;        /* [N] */
    const float* tbl[4];      /* [Q, D[s]]  gather: in */
    float* rows[4];           /* [N, D[s]]  gather: out, segsum: in */
    float* sums[4];           /* [Q, D[s]]  segsum: out */
    int D[4];
} ParrotLabelTablesDesc;

int parrot_label_tables_supported(long long N, int Q);
int parrot_label_gather(const ParrotLabelTablesDesc* desc, void* stream);
long long parrot_label_segsum_ws_floats(long long N, int Q, int Dtotal);
int parrot_label_segsum(const ParrotLabelTablesDesc* desc, float* ws, long long ws_floats, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mixture-density head of the training step (parrot_amd/csrc/gmmcost.hip): the Gaussian-mixture negative log-likelihood
 * (model.py:65-91) on the PRE-ACTIVATIONS of the three output heads (model.py:774-781) and its gradient, one pass over
 * the rows each way.  Row m, column o*K + k of mu / sig_hat (the order of ParrotSampleDesc::Wmu):
 *   sig_ok = exp(sig_hat_ok) + eps,   pi_k = softmax(co_hat)_k + eps,
 *   a_k    = log pi_k - 1/2 sum_o [ (y_o - mu_ok)^2 / sig_ok^2 + 2 log sig_ok + log 2 pi ]
 *   parrot_gmm_cost_fwd:  nll[m] = -logsumexp_k a_k (max-shifted, model.py:37-41),  pi_out[m,k] = pi_k (may be NULL),
 *                         logr[m,k] = a_k + nll[m]  (log responsibility; [M, K] contiguous, saved for the backward call)
 *   parrot_gmm_cost_bwd:  with r_k = exp(logr[m,k]), p = softmax(co_hat), q_k = -r_k / pi_k:
 *                         dmu[m,ok]      = rowscale[m] * ( - r_k (y_o - mu_ok) / sig_ok^2 )
 *                         dsig_hat[m,ok] = rowscale[m] * r_k (1 / sig_ok - (y_o - mu_ok)^2 / sig_ok^3) exp(sig_hat_ok)
 *                         dco_hat[m,j]   = rowscale[m] * p_j (q_j - sum_k p_k q_k)
 * rowscale is a device array [M] (mask, mask sum and upstream gradient folded in by the caller; no host read).  Leading
 * dimensions in floats, at least the row's width; no alignment beyond 4 bytes.  The gradients' address ranges may overlap
 * neither an input's nor each other's (PARROT_ERR_BADARG).  A row with rowscale[m] == 0 gets gradient rows of exactly 0.0
 * whatever its operands hold.
 * M, O, K >= 1; K > 64 is PARROT_ERR_UNSUPPORTED.  No allocation, no synchronisation, no atomics: the same bits every run.
 * ------------------------------------------------------------------------------------------ */
int parrot_gmm_cost_fwd(const float* y, int ldy, const float* mu, int ldmu, const float* sig_hat, int ldsig,
                        const float* co_hat, int ldco, long long M, int O, int K, float eps, float* nll, float* pi_out,
                        int ldpi, float* logr, void* stream);
int parrot_gmm_cost_bwd(const float* y, int ldy, const float* mu, int ldmu, const float* sig_hat, int ldsig,
                        const float* co_hat, int ldco, const float* logr, const float* rowscale, long long M, int O, int K,
                        float eps, float* dmu, int lddmu, float* dsig_hat, int lddsig, float* dco_hat, int lddco,
                        void* stream);

/* Weight-norm fold of a SampleRNN Linear (sampleRNN/lib/ops.py:101-110: `W * (g / W.norm(2, axis=0))`), SURVEY 8b's K9:
 *   samplernn_weightnorm_fold:      W_eff[k][n] = W[k][n] * g[n] / ||W[:, n]||_2;  norm[n] = ||W[:, n]||_2 (may be NULL)
 *   samplernn_weightnorm_fold_bwd:  dg[n] (+)= sum_k dW_eff[k][n] W[k][n] / norm[n]
 *                                   dW[k][n] (+)= g[n] / norm[n] * (dW_eff[k][n] - W[k][n] * sum_k' dW_eff[k'][n] W[k'][n] / norm[n]^2)
 * Row-major [K, N] matrices with leading dimensions ld / ldo / ldd / lddw >= N; ws: samplernn_weightnorm_ws_floats(N)
 * floats of scratch (partial column sums, added in a fixed order: no atomics). */
long long samplernn_weightnorm_ws_floats(int N);
int samplernn_weightnorm_fold(const float* W, int ld, const float* g, float* W_eff, int ldo, float* norm, float* ws, int K, int N,
                              void* stream);
int samplernn_weightnorm_fold_bwd(const float* W, int ld, const float* g, const float* norm, const float* dW_eff, int ldd,
                                  float* dW, int lddw, float* dg, float* ws, int K, int N, int accumulate_w, int accumulate_g,
                                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Conditional three-tier SampleRNN generation: the per-sample loop of generate_and_save_samples
 * (sampleRNN/models/conditional/three_tier.py:794-832) and the three Theano functions it calls
 * (getting_generation_functions, :703-734) as one device-resident launch sequence per 80-sample
 * period, replayed from a hipGraph.  All weights are the EFFECTIVE weights (weight norm,
 * ops.py:101-110, folded by the caller), row-major [in, out].  emb_tbl = Embedding folded with
 * SampleLevel.L1_PrevSamples: emb_tbl[pos][q][:] = Embedding[q] . W1[pos*EMB:(pos+1)*EMB, :].
 * temperature = 0 -> argmax (softmax_and_argmax, ops.py:296-297; lowest index on ties);
 * temperature > 0 -> multinomial draw from a seeded counter-based generator (not Theano's MRG stream).
 * draw_mode: how such a draw finds its code among the terms e_q = expf((logit_q - max) / temperature), on every path
 * (launches, the persistent sample kernel, row groups, starts, resumed segments, per-utterance draws); both modes see the
 * same uniforms u01, and argmax (temperature <= 0) is the same in both.
 *   0 (sequential, the default; a zeroed field): one lane adds the Q terms one after the other in float32 -- once for the
 *     total, once to find the first code with u01 * total < running sum.  The samples every earlier version drew.
 *   1 (scan): one 64-lane wave; Q must be a multiple of 64 (PARROT_ERR_BADARG otherwise).  Lane l owns the n = Q / 64
 *     contiguous codes n l + j and adds them left to right (p_l); an inclusive Hillis-Steele scan with offsets 1, 2, 4, 8
 *     inside each row of 16 lanes gives w_l (a lane without a source adds nothing); the row totals T_k = w_{16k+15} are
 *     chained R_0 = T_0, R_1 = R_0 + T_1, R_2 = R_1 + T_2 and s_l = w_l in row 0, R_{k-1} + w_l in row k; total = s_63,
 *     u = u01 * total; l* = the lowest lane with u < s_l (none: the pick is Q - 1); inside l* the terms are added one at a
 *     time to s_{l*-1} (0 for lane 0) and the first code with u < c is the pick (none: the lane's last code).  Every add
 *     is one float32 addition in exactly this order, so the pick is a function of the logits, the temperature and u01
 *     alone, the same on both kernel paths.  About 20 dependent operations instead of 2 Q; a sum has at most 14 roundings
 *     behind it instead of Q, so the pick agrees with the exact CDF wherever u01 is further than 2^-17 from a boundary
 *     (sequential: 2^-14), and terms below 2^-24 of the total are not lost.  A few draws per ten thousand differ from
 *     mode 0's by one code.
 *   Any other value: PARROT_ERR_BADARG.
 * top_k: a draw at temperature > 0 is taken among the k most likely codes, in both modes and on every path.
 *   The kept set is the k codes that come first when the codes are ordered by logit descending, then by code index
 *   ascending: a tie at the cut-off goes to the lower index, the argmax's rule.  A kept code's term is e_q as above, every
 *   other code's is 0.0f; the max, the key, the counter, the uniform, the comparison u01 * total < running sum and the order
 *   of the float32 additions (the walk over all Q codes; the tree of mode 1) are unchanged -- adding 0.0f is exact.  Where no
 *   code satisfies the comparison (u01 can be exactly 1.0) the pick is the highest kept code: in mode 0 the highest of all, in
 *   mode 1 the highest kept code not above the code that falls through without truncation (Q - 1; the last code of lane l*).
 *   top_k = 1 at any temperature > 0 therefore picks the argmax code.  0 (a zeroed field) or >= Q: no truncation, the samples
 *   and the executed instructions of the pick are those of a build without the field.  < 0: PARROT_ERR_BADARG.  1 .. Q-1
 *   with Q > 256: PARROT_ERR_UNSUPPORTED.  At temperature <= 0 the pick is the argmax and top_k is ignored.
 * top_p (nucleus; no field of the descriptor, which has no spare word: samplernn_generate_set_top_p below): for one draw with
 *   logits lg[0..Q-1] and temperature > 0,
 *   1. the terms are e_q as above; if top_k is active its kept set K is taken first, exactly as above, otherwise K is all codes;
 *   2. the codes of K are ordered by logit descending, then by code index ascending (top_k's order, the argmax's tie rule),
 *      tot_K is the mass of K, and the nucleus is the shortest prefix q_1 .. q_m of that order whose mass is >= p * tot_K;
 *      m >= 1 always, and a tie at the cut-off goes to the lower indices;
 *   3. every code outside the nucleus gets the term 0.0f;
 *   4. everything else is what a top_k draw with k = m does: the same max, key, counter and 24-bit u01, the same comparison
 *      u01 * tot < c, the same order of float32 additions (the walk over all Q codes in mode 0, the tree of mode 1) and the
 *      same fall-through picks (the highest kept code; in mode 1 the highest kept code not above the code the scan falls
 *      through to);
 *   5. so a draw with top_p = p is indistinguishable from a draw with top_k = m.
 *   The masses that find m are float32 sums of the non-negative terms in an order fixed per draw mode: a lane of the selecting
 *   wave adds its codes left to right (codes l, l + 64, l + 128, l + 192 in mode 0; 4 l .. 4 l + 3, or l Q/64 .. with Q < 256,
 *   in mode 1), and the 64 lane sums are added as a fixed tree -- lanes l and l^1, then l^2, then the mirror inside each
 *   half-row of 8, then inside each row of 16, then rows (0 + 1) + (2 + 3).  The bar is the float32 product p * tot_K.  A tree
 *   of round-to-nearest adds is monotone in every input, so the mass above a threshold is monotone in the threshold and the
 *   cut is found by binary search.  m equals the exact (real-number) m whenever every prefix mass of the exact order lies
 *   farther than 2^-14 from p, as a fraction of tot_K; for the same logits and draw mode the launch path and the persistent
 *   kernel keep the same set.  Not promised: the same m in both draw modes inside that margin.
 *   0.0 or >= 1.0: off, and the pick runs the instructions of a build without it.  < 0 or NaN: PARROT_ERR_BADARG.  Strictly
 *   between 0 and 1 with Q > 256: PARROT_ERR_UNSUPPORTED.  At temperature <= 0 the pick is the argmax and top_p is ignored; a
 *   very small p gives m = 1, the argmax.
 * samples: [B, BFS*T] int32, first BFS entries = Q/2 set by the caller; big_h / frm_h hold the
 * initial states (learned h0) on entry and the final states on return.  The weight buffers must not change during a
 * plan's life: create makes fragment-major copies of the tiers' matrices for the step kernel (single-GRU tiers) and, on the
 * persistent path, composes everything in front of L2's ReLU through W2 once (emb_tbl[pos] . W2, frm_Wout_i . W2,
 * frm_bout_i . W2 + b2; round 5) -- the sample kernel then has no L2 product.
 * A run need not be one rectangle of T frames: samplernn_generate_run_segment (below) runs any number of periods up to
 * T-1 and resumes from where the last call ended, with the buffers of this descriptor used as a ring.
 * ------------------------------------------------------------------------------------------ */
typedef struct SampleRnnGenDesc {
    int B, D, T, Q, FS, BFS, feat_dim;
    /* The descriptor has no spare word and its size and offsets are part of the ABI, so top_k shares the four bytes that
     * were `int use_graph` (a flag: 0 or 1).  On the little-endian hosts this library runs on, a caller compiled against
     * the earlier header still sets use_graph and leaves top_k = 0. */
    short use_graph, top_k;
    float temperature; int draw_mode;
    unsigned long long seed;
    const float* big_Win_frames; const float* big_Win_feats; const float* big_bin; /* [BFS,D],[feat,D],[D] */
    const float* big_U; const float* big_bU; const float* big_Wg; const float* big_Wc; /* [D,3D],[3D],[D,2D],[D,D] */
    const float* big_Wout; const float* big_bout;                                  /* [D,(BFS/FS)*D] */
    const float* frm_Win; const float* frm_bin;                                    /* [FS,D],[D] */
    const float* frm_U; const float* frm_bU; const float* frm_Wg; const float* frm_Wc;
    const float* frm_Wout; const float* frm_bout;                                  /* [D,FS*D] */
    const float* emb_tbl;                                                          /* [FS,Q,D] */
    const float* W2; const float* b2; const float* W3; const float* b3; const float* W4; const float* b4;
    const float* features;   /* [T,B,feat_dim] time-major */
    int* samples;            /* [B,BFS*T] */
    float* big_h; float* frm_h;            /* [B,D] */
    /* scratch */
    float* xf_big; float* xf_frm; float* feat_cur; float* gru_in; float* P; float* z; float* r; float* rh;
    float* big_out; float* frame_out; float* o1; float* o2; float* o3; float* logits;
    int* tbase;
    /* Stacked / LSTM tiers (three_tier.py:147-169 allows RNN_TYPE = 'LSTM' and N_RNN in 1..5; stackedGRU / stackedLSTM,
     * sampleRNN/lib/ops.py:612-777, 823-989; with skip connections: samplernn_generate_set_skip_stacks below).  n_rnn = 0
     * keeps the single-GRU fields above.
     * Otherwise, per tier and layer k < n_rnn, four pointers:
     *   GRU  (lstm = 0): { Input.W [D,3D], Input.b [3D], Recurrent_Gates [D,2D], Recurrent_Candidate [D,D] }
     *   LSTM (lstm = 1): { Input.W [D,4D], b [4D], Recurrent_Gates [D,4D], NULL }   (gate order i | f | o | g)
     * and the layer states big_hs / frm_hs [k] ([B,D]; initial state on entry, final on return) plus, for LSTM, the cell
     * states big_cs / frm_cs [k].  P must then hold B*4D floats, gate_ws B*4D floats (LSTM gate scratch), and
     * layer_tmp B*D floats. */
    int n_rnn, lstm;
    const float* big_L[5][4];
    const float* frm_L[5][4];
    float* big_hs[5]; float* big_cs[5];
    float* frm_hs[5]; float* frm_cs[5];
    float* gate_ws; float* layer_tmp;
    /* Optional workspace of the persistent-thread sample kernel (parrot_amd/csrc/sr_persist.hip): at least
     * samplernn_persist_floats(desc) floats (create initialises it; it belongs to ONE plan).  With it (B <= 32, D in {256, 512, 1024},
     * Q = 256, a 256-CU device) the FS sample steps between two frame-tier steps run as ONE launch: each XCD takes four
     * streams through the whole sample-level MLP with its weights held in LDS / registers and hand-offs that stay inside
     * the XCD's L2.  NULL or a non-qualifying configuration: five launches per sample as before.
     * PARROT_SR_PERSIST_GROUPS = G (1 .. 8, default 1; read by samplernn_persist_floats and create) lifts the batch limit to
     * B <= 32 G: one launch then takes the batch in ceil(B / 32) row groups of 32 streams, one after the other, with the
     * weights loaded once; the workspace grows with the group count. */
    float* persist_ws;
    long long persist_ws_floats;
    /* Optional: several utterances one after the other in each stream (three_tier.generate_packed).  starts [T][B],
     * device memory, read inside the loop: starts[f][b] != 0 means that stream b begins a new utterance at big frame f and
     * that slot f - 1 is that utterance's Q/2 prefix.  The first launch of such a period then rewrites, for the flagged
     * streams only, samples[b][BFS (f-1) .. BFS f) = Q/2, every state of row b that outlives a period (big_h / frm_h, or
     * big_hs / frm_hs and big_cs / frm_cs of every layer) from the learned initial states below, the row's share of the
     * next frame's gate product and, on the persistent path, the launch-to-launch carry of the row's team (invalidated:
     * that period's first sample launch reads its history from `samples`).  From there on the stream computes what a run
     * of its own computes.  starts[0] is never read.  NULL: nothing of this is launched.
     * big_h0 / frm_h0: [max(n_rnn, 1)][H0_MULT * D] learned initial states (BigFrameLevel.h0 / FrameLevel.h0), H0_MULT = 2
     * for LSTM tiers whose rows are [s | c], else 1.  Both are required when starts is set (PARROT_ERR_BADARG otherwise);
     * the caller still fills big_h / frm_h (...) with them for the first utterance of every stream. */
    const int* starts;
    const float* big_h0; const float* frm_h0;
} SampleRnnGenDesc;

/* Floats of persist_ws a plan for this descriptor needs (it grows with the row groups the batch takes); 0 when the
 * configuration does not qualify. */
long long samplernn_persist_floats(const SampleRnnGenDesc* desc);
/* Row groups of 32 streams per launch of the plan's persistent sample kernel: ceil(B / 32); 0 when the plan is not
 * persistent. */
int samplernn_generate_persist_groups(void* plan);
/* The same arithmetic without a device or a plan: the row groups a batch of B streams would take when at most max_groups
 * are allowed (PARROT_SR_PERSIST_GROUPS; values outside 1 .. 8 are clamped to that range), or 0 when B < 1 or
 * B > 32 * max_groups -- such a batch runs on launches. */
int samplernn_persist_groups_dry(int B, int max_groups);
int samplernn_generate_create(const SampleRnnGenDesc* desc, void** plan);
int samplernn_generate_run(void* plan, void* stream);
/* A run in segments: the plan's buffers as a ring of T slots.  n_periods in 1 .. T-1, else PARROT_ERR_BADARG.
 *   resume = 0: what samplernn_generate_run does, for n_periods periods instead of T-1 -- the caller has set the prefix slot
 *     and the initial states; slots 1 .. n_periods are generated from features[1 .. n_periods] (and starts[1 .. n_periods]).
 *     samplernn_generate_run(plan, stream) is samplernn_generate_run_segment(plan, T-1, 0, stream).
 *   resume = 1: continues the run the plan executed last (PARROT_ERR_BADARG on a plan that has not run).  A small launch in
 *     front of the first period reads on the device where that run ended (tbase / BFS - 1, whatever its n_periods was),
 *     copies that slot of every stream to slot 0, sets tbase back to BFS, re-keys the persistent kernel's carry and adds the
 *     samples moved past to the plan's draw origin; then slots 1 .. n_periods are generated from features[1 .. n_periods]
 *     and, on packed plans, starts[1 .. n_periods] (a start at frame 1 overwrites the moved slot with the Q/2 prefix).
 *     Nothing else is reset: the tier states, the next frame's gate product and, on packed plans, the h0 . Wg rows of the
 *     first run stay.  The caller reads slots 1 .. n_periods of `samples` (after samplernn_generate_status, which
 *     synchronises) and writes the next segment's frames before it calls again.
 * The segments of a run compute, bit for bit, the samples of the same run in one piece: seeded draws (temperature > 0) are
 * keyed by the sample's run index = draw origin + index in the buffer, and resume = 0 sets the origin to 0 -- together
 * with the stream and the plan's seed by default, or, after samplernn_generate_set_utterance_draws (below), counted from
 * the utterance's own prefix slot and hashed with the utterance's own seed.  Every segment replays the plan's two
 * captured graphs (eight periods, one period); nothing is captured per segment. */
int samplernn_generate_run_segment(void* plan, int n_periods, int resume, void* stream);
/* Per-utterance seeds and temperatures.  utt_seed [T][B] (unsigned long long), utt_temp [T][B] (float): device memory,
 * indexed like `starts` (ring rows), owned by the caller for the plan's life.  Row f holds what an utterance that begins at
 * big frame f draws with.  The plan keeps one entry {seed, off, temperature} per stream: a run with resume = 0 sets every
 * entry from row 1 with off = 0 (the stream's first utterance has its prefix in slot 0); a start flagged at (f, b) sets
 * entry b from row f with off = the run index (draw origin + index in the buffer) of the first sample of slot f - 1; a
 * resumed segment leaves the entries alone.  The draw of buffer index t in stream b then hashes
 * seed_b ^ K1 (origin + t - off_b + 1) -- the counter is the sample's index in the utterance's own buffer, prefix included,
 * and there is no stream term -- through the same finaliser and the same float32 inverse-CDF arithmetic as the default
 * key, with temperature_b (<= 0: argmax, lowest index on ties) in place of the descriptor's.  With off = 0 and
 * seed_b = s ^ K2 (b + 1) that is the default draw of plan seed s, bit for bit (K1 = 0x9E3779B97F4A7C15,
 * K2 = 0xBF58476D1CE4E5B9).  An utterance's samples then depend on the model, the plan's shape, the carrying stream and
 * the utterance's features, seed and temperature -- not on its slot, the segment boundaries or its neighbours.
 * PARROT_ERR_BADARG for a null plan or pointer (checked before any device call) and for a plan that has run: the period
 * graphs hold the pointers by value. */
int samplernn_generate_set_utterance_draws(void* plan, const unsigned long long* utt_seed, const float* utt_temp);
/* Per-utterance top-k.  utt_top_k [T][B] (int): device memory, indexed and owned like utt_temp; row f holds the top_k of an
 * utterance that begins at big frame f, with the meaning of SampleRnnGenDesc::top_k (<= 0 or >= Q: no truncation).  The
 * entry of a stream takes it wherever it takes the seed and the temperature, so the streams of one plan -- and the four
 * rows of one team of the persistent kernel -- may mix truncations as they mix temperatures.  Valid only after
 * samplernn_generate_set_utterance_draws, and refused once the plan has run (PARROT_ERR_BADARG for either, and for a null
 * plan or pointer; no device call); PARROT_ERR_UNSUPPORTED when Q > 256.  Without it every utterance takes the descriptor's
 * top_k. */
int samplernn_generate_set_utterance_top_k(void* plan, const int* utt_top_k);
/* The plan's top_p (see top_p above; a new plan's is 0.0 = off).  PARROT_ERR_BADARG for a null plan, for top_p < 0 or NaN
 * and for a plan that has run (the period graphs hold the value); PARROT_ERR_UNSUPPORTED for 0 < top_p < 1 with Q > 256.
 * No device call. */
int samplernn_generate_set_top_p(void* plan, float top_p);
/* Per-utterance top_p.  utt_top_p [T][B] (float): device memory, indexed and owned like utt_temp; row f holds the top_p of an
 * utterance that begins at big frame f (not strictly between 0 and 1: no nucleus).  The entry of a stream takes it wherever
 * it takes the seed, the temperature and top_k, so the streams of one plan -- and the four rows of one team of the
 * persistent kernel -- may mix nuclei as they mix truncations and temperatures.  Valid only after
 * samplernn_generate_set_utterance_draws, and refused once the plan has run (PARROT_ERR_BADARG for either, and for a null
 * plan or pointer; no device call); PARROT_ERR_UNSUPPORTED when Q > 256.  Without it every utterance takes the plan's top_p. */
int samplernn_generate_set_utterance_top_p(void* plan, const float* utt_top_p);
/* The plan's min_p (a new plan's is 0.0 = off).  For one draw with float32 logits lg[0..Q-1], temperature T > 0 and
 * 0 < min_p <= 1:
 *   1. e_q = expf((lg_q - best) / T) as the draw computes it, in float32; a code is kept iff e_q >= min_p, a float32 compare.
 *      The argmax has e = 1.0f exactly, so the set is never empty; min_p = 1 keeps exactly the codes whose term is 1.0f (the
 *      maxima);
 *   2. composition: the kept set is top_k's set, intersected with the nucleus of top_k's set, intersected with min-p's set.
 *      The nucleus is computed exactly as without min_p; min-p is applied last (temperature -> top-k -> top-p -> min-p).
 *      e_q / e_max does not change under renormalisation, so min-p commutes with top-k.  In exact arithmetic each of the
 *      three sets is a prefix of the order "logit descending, index ascending", so the intersection is the shortest of them:
 *      a draw with any combination is a draw with top_k = m;
 *   3. every code outside the kept set gets the term 0.0f in the same sums, with the same uniform, in both draw modes, and
 *      the fall-through picks go to the highest kept code, exactly as for top_k.
 *   The kept set equals the exact one whenever every ratio e_q / e_max lies farther than 2^-18 (relative) from min_p.
 *   0.0: off, and the pick runs the instructions of a build without it (the kernels treat any value outside (0, 1] as off).
 *   < 0, > 1 or NaN: PARROT_ERR_BADARG, as for a null plan and for a plan that has run (the period graphs hold the value);
 *   active with Q > 256: PARROT_ERR_UNSUPPORTED.  At temperature <= 0 the pick is the argmax and min_p is ignored.  No device
 *   call. */
int samplernn_generate_set_min_p(void* plan, float min_p);
/* Per-utterance min_p.  utt_min_p [T][B] (float): device memory, indexed and owned like utt_top_p; row f holds the min_p of
 * an utterance that begins at big frame f (outside (0, 1]: off).  The entry of a stream takes it wherever it takes the seed,
 * the temperature, top_k and top_p, so the four rows of one team of the persistent kernel may mix every kind of truncation.
 * Valid only after samplernn_generate_set_utterance_draws, and refused once the plan has run (PARROT_ERR_BADARG for either,
 * and for a null plan or pointer; no device call); PARROT_ERR_UNSUPPORTED when Q > 256.  Without it every utterance takes
 * the plan's min_p. */
int samplernn_generate_set_utterance_min_p(void* plan, const float* utt_min_p);
/* Forced samples (teacher forcing, priming).  forced [B][BFS * T] (int): device memory, owned by the caller for the plan's
 * life, indexed exactly like `samples` -- the same ring and the same buffer index t; a run in segments restages it per
 * segment, as it restages `features`.  Where forced[b][t] lies in 0 .. Q-1 the sample step at buffer index t of stream b
 * computes its logits as always and then takes forced[b][t] as the sample instead of its pick: that code is written to
 * `samples` and enters the following steps, the frame and big-frame tiers and a resumed segment like any sample.  Any other
 * value (-1 is the documented one) means that the step picks freely; an out-of-range value never indexes a table.  Slot 0
 * of a run (the prefix slot) is never read.  The draw counter stays the sample's index: a forced step consumes no uniform,
 * a free step after a prompt uses the uniform of its own index, so forcing a run's own earlier output reproduces that run
 * bit for bit.  Independent of every draw setting and of samplernn_generate_set_log_probs.  PARROT_ERR_BADARG for a null plan
 * or pointer and for a plan that has run (the period graphs hold the pointer by value); no device call. */
int samplernn_generate_set_forced(void* plan, const int* forced);
/* Per-sample log-probabilities.  logp [B][BFS * T] (float): device memory, owned and indexed like `forced`.  Every sample
 * step writes logp[b][t] = logits[s] - max - log(sum_q exp(logits[q] - max)), s = the code the step wrote to `samples`
 * (forced or picked): the natural logarithm, in float32, of the MODEL's probability of s -- temperature 1, no truncation,
 * whatever the step draws with; the quantity the training cost averages.  Slot 0 is not written.  PARROT_ERR_BADARG for a
 * null plan or pointer and for a plan that has run; no device call. */
int samplernn_generate_set_log_probs(void* plan, float* logp);
/* What each draw kept.  draw_logp [B][BFS * T] (float) and kept [B][BFS * T] (int): device memory, owned and indexed like
 * `logp`; both required.  Every sample step writes kept[b][t] = the size of the set its pick was drawn from -- 1 on an argmax
 * step (temperature <= 0), Q on an untruncated draw, else the number of codes top_k, top_p and min_p left; a forced step
 * reports the set its pick was drawn from, like any other -- and draw_logp[b][t] = (logits[s] - max) / T - log(sum of the kept
 * codes' terms), s = the code the step wrote to `samples`: the natural logarithm, in float32, of the probability of s under
 * the distribution the step drew from.  -inf where s is outside the kept set (a forced code the truncation dropped, or a
 * forced code that is not the argmax on an argmax step), 0 for the argmax on an argmax step.  The mass is a fixed tree of
 * float32 adds, so the same logits and settings give the same bits.  Slot 0 is not written.  On the launch path: any Q
 * untruncated, Q <= 256 truncated.  Independent of every draw setting, of forced samples and of log_probs.
 * PARROT_ERR_BADARG for a null plan or pointer and for a plan that has run; no device call. */
int samplernn_generate_set_draw_stats(void* plan, float* draw_logp, int* kept);
/* Skip-connection stacks (--skip_conn True: Graves' stacks, sampleRNN/lib/ops.py:650-695, 861-880).  In such a stack every
 * layer above the first reads [h_{k-1} ; x], x = the stack's input, and the stack's output is sum_k h_k . S_k + bS instead
 * of the top layer's state.  The descriptor does not change; a plan with n_rnn >= 2 takes the rest through this struct:
 *   big_S / frm_S [k], k < n_rnn: [D, D] the effective (weight-norm folded) out-skip matrix of layer k + 1
 *     ('<tier>.GRU.outskip<k+1>y', '<tier>.LSTM<k+1>.outskip<k+1>y');
 *   big_bS / frm_bS: [D] the bias of the first out-skip (the others have none);
 *   big_sum / frm_sum: [B, D] scratch for the summed output, owned by the caller for the plan's life.
 * With the setter in force, slot 0 of big_L[k] / frm_L[k] for k >= 1 is the [2D, N] Input matrix of
 * '<tier>.GRU<k+1>+inpskip' / '<tier>.LSTM<k+1>+inpskip' (N = 3D for GRU, 4D for LSTM): rows 0 .. D-1 multiply h_{k-1},
 * rows D .. 2D-1 multiply x.  Weight norm scales each column over all 2D rows: fold it as one matrix.  The step jobs of
 * those layers carry one more K segment, and one more job per tier step makes the sum (f32) into big_sum / frm_sum, which
 * the tier's output projection then reads in place of the top state.  Everything else -- the sample steps, the draws,
 * packing, segments, forcing, log-probabilities -- is what it is without the setter.
 * PARROT_ERR_BADARG for a null plan, struct or pointer (S of layers >= n_rnn are not read); PARROT_ERR_UNSUPPORTED for a
 * plan with n_rnn < 2 (the single-GRU plan has n_rnn = 0, and no one-layer stack has skip connections);
 * PARROT_ERR_BADARG for a plan that has run (the period graphs hold the pointers by value).  A refused call leaves the plan
 * as it was.  No device call. */
typedef struct SampleRnnSkipStacks {
    const float* big_S[5]; const float* frm_S[5];
    const float* big_bS; const float* frm_bS;
    float* big_sum; float* frm_sum;
} SampleRnnSkipStacks;
int samplernn_generate_set_skip_stacks(void* plan, const SampleRnnSkipStacks* skip);
/* Conditioning frames from device memory.  src [src_rows][src_ld] (float, src_ld >= feat_dim; a decoder's frame rows have
 * src_ld = 64) and index [rows][B] (int): device memory.  For every r < rows and b < B, features[first + r][b][0 .. feat_dim)
 * of the plan's own `features` buffer (SampleRnnGenDesc::features) becomes src[index[r][b] * src_ld + 0 .. feat_dim), a
 * bit-exact copy, where 0 <= index[r][b] < src_rows, and zeros otherwise: a negative entry is the documented "idle slot",
 * and no entry, whatever it holds, makes the kernel read outside src.  Nothing outside rows first .. first + rows - 1 is
 * written.  One launch on `stream`, ordered like any other work there: stage, then run the segment that reads the rows.
 * Because the plan's buffer is written, every generation path sees the frames (persistent kernel, row groups, launches,
 * resumed segments); the entry may be called at any time in a plan's life, and SampleRnnGenDesc is unchanged.
 * PARROT_ERR_BADARG, before any device call, for a null plan, src or index, first < 0, rows < 1, first + rows > T,
 * src_ld < feat_dim, src_rows < 1. */
int samplernn_generate_stage_features(void* plan, const float* src, long long src_rows, int src_ld, const int* index, int first,
                                      int rows, void* stream);
/* 1 when the plan's sample steps run on the persistent-thread kernel. */
int samplernn_generate_is_persistent(void* plan);
/* Waits for the device and returns 0, or a non-zero fault code when a persistent sample kernel gave up (a team of
 * workgroups was incomplete or timed out): the samples of that run are invalid.  Always 0 on the launch path. */
int samplernn_generate_status(void* plan);
int samplernn_generate_destroy(void* plan);

#ifdef __cplusplus
}
#endif
#endif /* PARROT_HIP_H */

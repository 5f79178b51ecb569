// extern "C" entry points that are single operations (the scan plans live in plans.hip).
#include "../../include/parrot_hip.h"
#include "attention.h"
#include "biggemm.h"
#include "elementwise.h"
#include "quantize.h"
#include "skinny.h"
#include "switches.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

static int gemm_target_wgs() {
    return 1024;  // 8-wave kernel: 1024..4096 measure the same; fewer slices = less partial-sum traffic
}

// parrot_set_gemm_precision (process-wide; plans override per thread).  Default since round 6: the split-bf16 products
// (PARROT_PRECISION_BF16X3: f32 operands, f32-grade results, 1.7-1.9 x the f32-input MFMA kernel's rate);
// PARROT_GEMM_PRECISION=f32 in the environment restores the f32-input matrix instructions for everything.
static int gemm_default_mode() {
    const char* e = env_str("PARROT_GEMM_PRECISION");
    if (e && (!strcmp(e, "f32") || !strcmp(e, "0"))) return PARROT_PRECISION_F32;
    if (e && (!strcmp(e, "bf16") || !strcmp(e, "1"))) return PARROT_PRECISION_BF16;
    return PARROT_PRECISION_BF16X3;
}
static std::atomic<int> g_gemm_bf16{gemm_default_mode()};
static thread_local int t_gemm_bf16 = -1;   // BgPrecisionScope (-1: follow the process-wide mode)
BgPrecisionScope::BgPrecisionScope(int bf16) : saved(t_gemm_bf16) { t_gemm_bf16 = bf16 < 0 ? saved : (bf16 ? 1 : 0); }
BgPrecisionScope::~BgPrecisionScope() { t_gemm_bf16 = saved; }

extern "C" {

int parrot_set_gemm_precision(int mode) { PH_ENTRY();
    if (mode != PARROT_PRECISION_F32 && mode != PARROT_PRECISION_BF16 && mode != PARROT_PRECISION_BF16X3) return PARROT_ERR_BADARG;
    g_gemm_bf16.store(mode, std::memory_order_relaxed);
    return 0;
}

int parrot_get_gemm_precision(void) { PH_ENTRY(); return g_gemm_bf16.load(std::memory_order_relaxed); }

const char* parrot_hip_version(void) { PH_ENTRY(); return "parrot_hip 0.5.0 gfx950"; }

int parrot_profile_begin(void) { PH_ENTRY();
    sk_profile_begin();
    return 0;
}

long long parrot_profile_end(double* total_us, double* flops, double* bytes) { PH_ENTRY();
    return sk_profile_end(total_us, flops, bytes);
}

long long parrot_profile_end2(double* total_us, double* flops, double* bytes, double* plain4) { PH_ENTRY();
    return sk_profile_end2(total_us, flops, bytes, plain4);
}

// Split-K workspace (products on different streams -- the weight-gradient GEMMs that run beside the backward scan,
// model.py's _backward -- never share partial tiles).  Where there is none the product runs unsplit.
static StreamScratch bg_workspace(0);

// Automatic split-K: the slice count bg_run plans for a product on kernel `bf16` (BgArgs::bf16: 0 / 1 the 128 x 128
// tile kernels, 2 bgh_kernel, 3 bgs_kernel) when the caller passes split_k <= 0.  One rule per tile family.  Pure host
// arithmetic: parrot_gemm_route reports what it returns.
static int bg_auto_split(int bf16, int M, int N, int K, int act, int nbatch) {
    // few output tiles but a long reduction (deferred weight gradients: K = T*B rows)
    // -> spread K over enough workgroups to fill 256 CUs.
    int bm, bn;
    bg_tile_shape(bf16, bm, bn);
    const long long tiles = (long long)ceil_div(M, bm) * ceil_div(N, bn) * nbatch;
    int split = 1;
    if (bf16 == 3) {
        // 256 x 256 tiles, one workgroup per CU, slices dealt to XCDs: a multiple of 8 slices whose workgroups fill
        // whole rounds of 256 best, at least 512 K rows per slice
        if (act == 0 && tiles < 256 && K >= 4096) {
            double best = -1.0;
            for (int sp = 8; sp <= 64 && K / sp >= 512; sp += 8) {
                const long long wgs = tiles * sp;
                const double eff = (double)wgs / (double)((wgs + 255) / 256 * 256);
                const double score = eff - 0.001 * sp;
                if (score > best) { best = score; split = sp; }
            }
        }
    } else if (bf16 == 2 && K >= 512 && tiles < 256) {
        // (tiles >= 256: the output tiles fill the chip by themselves -- the M = T*B readout products -- and a split
        // would only add a partial-sum pass larger than the operands: ADVICE r05)
        // 256 x 256 tiles, one workgroup per CU: the slice count whose workgroups fill whole rounds of 256 best
        // (at least two rounds, at most 16 slices, at least 1024 K rows per slice)
        double best = -1.0;
        for (int sp = 1; sp <= 16 && K / sp >= 1024; ++sp) {
            const long long wgs = tiles * sp;
            const double eff = (double)wgs / (double)((wgs + 255) / 256 * 256);
            const double score = eff - (wgs < 512 ? 0.25 : 0.0) - 0.002 * sp;
            if (score > best) { best = score; split = sp; }
        }
    } else if (act == 0 && tiles < 512 && K >= 512) {
        split = (int)((gemm_target_wgs() + tiles - 1) / tiles);
        const int maxs = K / 256 > 0 ? K / 256 : 1;
        if (split > maxs) split = maxs;
        if (split > 64) split = 64;
    }
    return split;
}

// The deterministic split-K workspace and the launch of one batched product (shared by parrot_gemm and
// parrot_gemm_bf16in).
static int bg_run(BgArgs a, int split_k, hipStream_t st) {
    const int M = a.M, N = a.N, nbatch = a.nbatch, act = a.act;
    const float* bias = a.bias;
    const int split = split_k > 0 ? split_k : bg_auto_split(a.bf16, M, N, a.K, act, nbatch);
    a.splitk = split;
    a.ws = nullptr;
    if (a.splitk > 1) {
        if (act != 0) return PARROT_ERR_BADARG;
        // Deterministic split-K: the slices write partial tiles to a library-owned workspace and a second kernel adds
        // them in slice order (results do not depend on scheduling).  The workspace grows on demand and is reused by
        // later calls in stream order.  Under stream capture or when the workspace cannot be had, the product runs
        // unsplit instead: there is no float-atomic combine any more.
        float* ws = bg_workspace.get(st, (size_t)nbatch * a.splitk * M * N);
        if (ws) {
            a.ws = ws;
            a.bias = nullptr;  // the reducer adds it
            int rc = bg_launch(a, st);
            if (rc) return rc;
            a.bias = bias;
            return bg_reduce_launch(a, st);
        }
        a.splitk = 1;
    }
    return bg_launch(a, st);
}

// Which kernel a parrot_gemm / parrot_gemm_gated call takes (PARROT_GEMM_ROUTE_*) under precision `mode`.  The one copy
// of the dispatch rule: gemm_impl launches what this returns and parrot_gemm_route reports it.  The pointers are only
// looked at for their alignment.
static int gemm_pick_kernel(const float* A, int lda, int transA, const float* B, int ldb, int transB, int M, int N, int K,
                            float alpha, int act, int nbatch, long long strideA, long long strideB, int split_k,
                            bool has_gate, int mode) {
    // the weight-streaming step kernel: plain x . W (+ bias, activation, accumulate) on at most 64 rows
    if (M <= 64 && !transA && nbatch == 1 && split_k <= 1 && alpha == 1.0f && !has_gate) return PARROT_GEMM_ROUTE_STEP;
    if (mode == PARROT_PRECISION_BF16) return PARROT_GEMM_ROUTE_BF16;
    if (mode == PARROT_PRECISION_BF16X3) {
        // split-bf16 products (bgs_kernel): f32 operands and f32-grade results on the bf16 matrix pipe.  Taken where the
        // 256 x 256 tile pays: both operands fetched as aligned 16-byte vectors, enough work; the rest stays on the
        // f32-input MFMA kernel.
        auto al = [](const float* p, long long ld) { return (((uintptr_t)p & 15) == 0) && (ld % 4 == 0); };
        const bool ok = act <= 1 && al(A, lda) && al(B, ldb) && (strideA % 4 == 0) && (strideB % 4 == 0) && M >= 128 && N >= 128 &&
                        K >= 64 && (!transA || M % 4 == 0) && (transA || K % 4 == 0) && (transB || N % 4 == 0) && (!transB || K % 4 == 0);
        if (ok) return PARROT_GEMM_ROUTE_BF16X3;
    }
    return PARROT_GEMM_ROUTE_F32;
}

static int gemm_mode_in_force() { return t_gemm_bf16 >= 0 ? t_gemm_bf16 : g_gemm_bf16.load(std::memory_order_relaxed); }

// BgArgs::bf16 of a big-kernel route
static int gemm_route_bf16(int route) {
    return route == PARROT_GEMM_ROUTE_BF16X3 ? 3 : route == PARROT_GEMM_ROUTE_BF16 ? 1 : 0;
}

static int gemm_impl(const float* A, int lda, int transA, const float* B, int ldb, int transB, float* C, int ldc,
                     int M, int N, int K, const float* bias, float alpha, int accumulate, int act, int nbatch,
                     long long strideA, long long strideB, long long strideC, int split_k, const float* gate, int ldg,
                     void* stream) {
    if (!A || !B || !C || M < 1 || N < 1 || K < 1 || nbatch < 1) return PARROT_ERR_BADARG;
    if (gate && (nbatch != 1 || ldg < N)) return PARROT_ERR_BADARG;
    // the step kernel adds C after the activation, the big kernels before it: the combination has no one meaning
    if (act != 0 && accumulate) return PARROT_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int route = gemm_pick_kernel(A, lda, transA, B, ldb, transB, M, N, K, alpha, act, nbatch, strideA, strideB, split_k,
                                       gate != nullptr, gemm_mode_in_force());
    if (route == PARROT_GEMM_ROUTE_STEP) {
        SkJob j;
        sk_linear_job(j, sk_seg(A, lda, B, ldb, K, transB ? 1 : 0), M, N, N, C, ldc, accumulate);
        j.act = act;
        j.bias = bias;
        SkLaunch L;
        int rc = sk_make_launch(L, &j, 1);
        if (rc) return rc;
        return sk_launch(L, st);
    }
    BgArgs a;
    a.A = A; a.B = B; a.C = C; a.bias = bias;
    a.M = M; a.N = N; a.K = K;
    a.sam = transA ? 1 : lda; a.sak = transA ? lda : 1;
    a.sbk = transB ? 1 : ldb; a.sbn = transB ? ldb : 1;
    a.ldc = ldc;
    a.batchA = strideA; a.batchB = strideB; a.batchC = strideC;
    a.nbatch = nbatch;
    a.accumulate = accumulate; a.alpha = alpha; a.act = act;
    a.gate = gate; a.ldg = ldg;
    a.bf16 = gemm_route_bf16(route);
    return bg_run(a, split_k, st);
}

int parrot_gemm(const float* A, int lda, int transA, const float* B, int ldb, int transB, float* C, int ldc,
                int M, int N, int K, const float* bias, float alpha, int accumulate, int act, int nbatch,
                long long strideA, long long strideB, long long strideC, int split_k, void* stream) { PH_ENTRY();
    return gemm_impl(A, lda, transA, B, ldb, transB, C, ldc, M, N, K, bias, alpha, accumulate, act, nbatch, strideA, strideB,
                     strideC, split_k, nullptr, 0, stream);
}

int parrot_gemm_gated(const float* A, int lda, int transA, const float* B, int ldb, int transB, float* C, int ldc,
                      int M, int N, int K, const float* gate, int ldg, void* stream) { PH_ENTRY();
    if (!gate) return PARROT_ERR_BADARG;
    return gemm_impl(A, lda, transA, B, ldb, transB, C, ldc, M, N, K, nullptr, 1.0f, 0, 0, 1, 0, 0, 0, 0, gate, ldg, stream);
}

int parrot_gemm_route(const float* A, int lda, int transA, const float* B, int ldb, int transB, int M, int N, int K,
                      float alpha, int act, int nbatch, long long strideA, long long strideB, int split_k, int has_gate,
                      int* kernel, int* slices) {
    // (no HIP call here, not even PH_ENTRY's: the query works without a device)
    if (!A || !B || !kernel || !slices || M < 1 || N < 1 || K < 1 || nbatch < 1) return PARROT_ERR_BADARG;
    if (has_gate && nbatch != 1) return PARROT_ERR_BADARG;
    const int route = gemm_pick_kernel(A, lda, transA, B, ldb, transB, M, N, K, alpha, act, nbatch, strideA, strideB, split_k,
                                       has_gate != 0, gemm_mode_in_force());
    int split = 1;
    if (route != PARROT_GEMM_ROUTE_STEP) {
        split = split_k > 0 ? split_k : bg_auto_split(gemm_route_bf16(route), M, N, K, act, nbatch);
        if (split > 1 && act != 0) return PARROT_ERR_BADARG;  // as bg_run
    }
    *kernel = route;
    *slices = split;
    return 0;
}

int parrot_step_launch_mode(int njobs, const int* M, const int* N, const int* K, const int* lstm_H, int* info) {
    // (no HIP call here: the query works without a device)
    if (!M || !N || !K || !info || njobs < 1 || njobs > SK_MAXJOB) return PARROT_ERR_BADARG;
    SkJob jobs[SK_MAXJOB];
    for (int q = 0; q < njobs; ++q) {
        if (M[q] < 1 || N[q] < 1 || K[q] < 1) return PARROT_ERR_BADARG;
        SkJob& j = jobs[q];
        // (shapes only: the jobs are laid out by sk_prepare, never launched, so their buffers stay null)
        if (lstm_H && lstm_H[q] > 0) {
            sk_lstm_job(j, M[q], lstm_H[q], nullptr, nullptr, nullptr, nullptr);
            j.N = N[q];  // (as given: sk_make_launch refuses a width other than 4 lstm_H)
        } else {
            sk_linear_job(j, M[q], N[q], N[q], nullptr, 0);
        }
        const float* aligned_base = reinterpret_cast<const float*>(uintptr_t(4096));  // (inspected for alignment only)
        j.nseg = 1;
        j.seg[0] = sk_seg(aligned_base, (K[q] + 3) & ~3, aligned_base, (N[q] + 3) & ~3, K[q], 0);
    }
    SkLaunch Lin, L;
    const int rc = sk_make_launch(Lin, jobs, njobs);
    if (rc) return rc;
    dim3 grid;
    size_t lds;
    int mbnb;
    sk_prepare(Lin, L, grid, lds, mbnb);
    info[0] = L.zmode; info[1] = mbnb; info[2] = (int)grid.x; info[3] = (int)grid.y; info[4] = (int)grid.z;
    for (int q = 0; q < njobs; ++q) info[5 + q] = L.tile_end[q];
    return 0;
}

int parrot_step_job(int epi, int M, int N, int H, int nseg, const float* const* A, const int* lda, const void* const* B,
                    const int* ldb, const int* K, int layout, int act, int accumulate, int force_tile, const float* bias,
                    const float* add, int ld_add, float* out, int ldo, const float* e0, const float* e1, float* o1, float* o2,
                    void* stream) { PH_ENTRY();
    if (!A || !lda || !B || !ldb || !K || !out || nseg < 1 || nseg > SK_MAXSEG || M < 1 || N < 1 || H < 1 || layout < 0 ||
        layout > 3 || act < 0 || act > SK_ACT_SIGMOID)
        return PARROT_ERR_BADARG;
    SkJob j;
    switch (epi) {
        case SK_EPI_LINEAR: sk_linear_job(j, M, N, H, out, ldo, accumulate ? 1 : 0); break;
        case SK_EPI_GRU_GATES:
            if (!e0 || !o1 || !o2 || N != 2 * H) return PARROT_ERR_BADARG;
            sk_gru_gates_job(j, M, H, e0, o1, o2, out);
            break;
        case SK_EPI_GRU_CAND:
            if (!e0 || !e1 || N != H) return PARROT_ERR_BADARG;
            sk_gru_cand_job(j, M, H, e0, e1, o1, out);
            break;
        case SK_EPI_BWD_RH:
            if (!e0 || !e1 || !o1 || N != H) return PARROT_ERR_BADARG;
            sk_bwd_rh_job(j, M, H, e0, e1, out, ldo, o1);
            break;
        case SK_EPI_LSTM:
            if (!e1 || !o1 || N != 4 * H) return PARROT_ERR_BADARG;
            sk_lstm_job(j, M, H, e1, o1, o2, out);
            break;
        default: return PARROT_ERR_BADARG;
    }
    j.nseg = nseg;
    for (int s = 0; s < nseg; ++s) {
        if (!A[s] || !B[s] || K[s] < 1) return PARROT_ERR_BADARG;
        j.seg[s] = sk_seg(A[s], lda[s], static_cast<const float*>(B[s]), ldb[s], K[s], layout);
    }
    j.act = act;
    j.bias = bias;
    j.add = add;
    j.ld_add = ld_add;
    SkLaunch L;
    const int rc = sk_make_launch(L, &j, 1);
    if (rc) return rc;
    L.force_tile = force_tile;
    return sk_launch(L, (hipStream_t)stream);
}

int parrot_to_bf16(const float* x, void* y, long long n, void* stream) { PH_ENTRY();
    if (!x || !y || n < 0) return PARROT_ERR_BADARG;
    return bg_to_bf16_launch(x, y, n, (hipStream_t)stream);
}

int parrot_gemm_bf16in_ex(const void* A, int lda, int transA, const void* B, int ldb, int transB, float* C, int ldc, int M,
                          int N, int K, const float* bias, int accumulate, int split_k, void* stream) { PH_ENTRY();
    if (!A || !B || !C || M < 1 || N < 1 || K < 1) return PARROT_ERR_BADARG;
    BgArgs a;
    a.A = reinterpret_cast<const float*>(A); a.B = reinterpret_cast<const float*>(B); a.C = C; a.bias = bias;
    a.M = M; a.N = N; a.K = K;
    a.sam = transA ? 1 : lda; a.sak = transA ? lda : 1;   // as parrot_gemm, in bf16 elements
    a.sbk = transB ? 1 : ldb; a.sbn = transB ? ldb : 1;
    a.ldc = ldc;
    a.batchA = a.batchB = a.batchC = 0;
    a.nbatch = 1;
    a.accumulate = accumulate; a.alpha = 1.0f; a.act = 0;
    a.gate = nullptr; a.ldg = 0;
    a.bf16 = 2;
    return bg_run(a, split_k, (hipStream_t)stream);
}

int parrot_gemm_bf16in(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                       int accumulate, int split_k, void* stream) {
    // A(m, k) at A[k * lda + m]: the caller's [K, M] matrix read as its transpose
    return parrot_gemm_bf16in_ex(A, lda, 1, B, ldb, 0, C, ldc, M, N, K, nullptr, accumulate, split_k, stream);
}

int parrot_tile_weights(const float* W, int rows, int cols, int ld, float* out, int mode, int lstm_H, void* stream) { PH_ENTRY();
    if (mode != 0 && mode != 1) return PARROT_ERR_BADARG;
    return sk_tile_weights_launch(W, rows, cols, ld, out, mode, lstm_H, (hipStream_t)stream);
}

int parrot_tile_weights_bf16(const float* W, int rows, int cols, int ld, void* out, int mode, int lstm_H, void* stream) { PH_ENTRY();
    if (mode != 0 && mode != 1 && mode != 2) return PARROT_ERR_BADARG;
    return sk_tile_weights_bf16_launch(W, rows, cols, ld, out, mode, lstm_H, (hipStream_t)stream);
}

int parrot_simple_norm_fwd(const float* x, int ldx, float* y, int ldy, float* sigma, long long R, int N, float eps,
                           float* add_dst, int ld_add, void* stream) { PH_ENTRY();
    if (!x || !y || !sigma) return PARROT_ERR_BADARG;
    return simple_norm_fwd_launch(x, ldx, y, ldy, sigma, R, N, eps, add_dst, ld_add, (hipStream_t)stream);
}

int parrot_simple_norm_bwd(const float* dy, int lddy, const float* y, int ldy, const float* sigma, float* dx,
                           int lddx, long long R, int N, float eps, int accumulate, void* stream) { PH_ENTRY();
    if (!dy || !y || !sigma || !dx) return PARROT_ERR_BADARG;
    return simple_norm_bwd_launch(dy, lddy, y, ldy, sigma, dx, lddx, R, N, eps, accumulate, (hipStream_t)stream);
}

int parrot_colsum(const float* x, long long M, int N, int ld, float* out, int accumulate, void* stream) { PH_ENTRY();
    return colsum_launch(x, M, N, ld, out, accumulate, (hipStream_t)stream);
}

int parrot_colsum_route(const float* x, long long M, int N, int ld, const float* out, int* info2) {
    // (no HIP call here, not even PH_ENTRY's: the query works without a device)
    if (!x || !info2 || M < 0 || N < 1) return PARROT_ERR_BADARG;
    const ColsumRoute r = colsum_route(x, M, N, ld, out);
    info2[0] = r.vec4;
    info2[1] = r.ysplit;
    return 0;
}

int parrot_gru_step_fwd(const float* h, const float* inputs, const float* gate_inputs, const float* mask,
                        const float* Wg, const float* Wc, float* h_out, float* z, float* r, float* rh,
                        float* c, int B, int H, void* stream) { PH_ENTRY();
    if (!h || !Wg || !Wc || !h_out || !z || !r || !rh || B < 1 || H < 1) return PARROT_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    SkJob j;
    SkLaunch L;
    sk_gru_gates_job(j, B, H, h, z, r, rh);
    j.nseg = 1;
    j.seg[0] = sk_seg(h, H, Wg, 2 * H, H, 0);
    j.add = gate_inputs; j.ld_add = 2 * H;
    int rc = sk_make_launch(L, &j, 1);
    if (rc) return rc;
    rc = sk_launch(L, st);
    if (rc) return rc;
    sk_gru_cand_job(j, B, H, h, z, c, h_out);
    j.nseg = 1;
    j.seg[0] = sk_seg(rh, H, Wc, H, H, 0);
    j.add = inputs; j.ld_add = H;
    j.mask = mask;
    rc = sk_make_launch(L, &j, 1);
    if (rc) return rc;
    return sk_launch(L, st);
}

int parrot_gru_step_bwd(const float* dh_out, const float* h, const float* mask, const float* Wg,
                        const float* Wc, const float* z, const float* r, const float* c, float* dh,
                        float* d_inputs, float* d_gate_inputs, int B, int H, void* stream) { PH_ENTRY();
    if (!dh_out || !h || !Wg || !Wc || !z || !r || !c || !dh || !d_inputs || !d_gate_inputs)
        return PARROT_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(dh, 0, sizeof(float) * (size_t)B * H, st);
    if (e != hipSuccess) return (int)e;
    GruStateBwdArgs ga;
    ga.nchain = 1; ga.B = B; ga.H = H;
    ga.chain[0].dh = dh_out; ga.chain[0].dh2 = nullptr; ga.chain[0].hprev = h; ga.chain[0].z = z; ga.chain[0].c = c;
    ga.chain[0].mask = mask; ga.chain[0].dC = d_inputs; ga.chain[0].dG = d_gate_inputs; ga.chain[0].dhprev = dh;
    int rc = gru_state_bwd_launch(ga, st);
    if (rc) return rc;
    SkJob j;
    SkLaunch L;
    sk_bwd_rh_job(j, B, H, h, r, d_gate_inputs + H, 2 * H, dh);
    j.nseg = 1;
    j.seg[0] = sk_seg(d_inputs, H, Wc, H, H, 1);
    rc = sk_make_launch(L, &j, 1);
    if (rc) return rc;
    rc = sk_launch(L, st);
    if (rc) return rc;
    sk_linear_job(j, sk_seg(d_gate_inputs, 2 * H, Wg, 2 * H, 2 * H, 1), B, H, H, dh, H, 1);
    rc = sk_make_launch(L, &j, 1);
    if (rc) return rc;
    return sk_launch(L, st);
}

static int gmm_attention_fwd_impl(const float* h1, const float* WattT, const float* batt, const float* kappa_prev,
                                  const float* ctx, float* a, float* b, float* kappa, float* phi, float* w, int B,
                                  int H, int A, int U, int E, int att_type, float eps, float alignment,
                                  float sharpening, float timing, int* sup, void* stream) {
    if (!h1 || !WattT || !kappa_prev || !ctx || !a || !b || !kappa || !phi || !w) return PARROT_ERR_BADARG;
    AttFwdArgs g{};
    g.sup_out = sup;
    g.h1 = h1; g.ldh = H; g.WattT = WattT; g.batt = batt; g.kappa_prev = kappa_prev; g.ctx = ctx;
    g.a_out = a; g.b_out = b; g.kappa_out = kappa; g.phi_out = phi; g.w_out = w; g.ldw = E;
    g.B = B; g.H = H; g.A = A; g.U = U; g.E = E; g.esplit = att_default_esplit(B, E);
    g.att_type = att_type; g.eps = eps; g.alignment = alignment; g.sharpening = sharpening; g.timing = timing;
    return att_fwd_launch(g, (hipStream_t)stream);
}

int parrot_gmm_attention_fwd(const float* h1, const float* WattT, const float* batt, const float* kappa_prev,
                             const float* ctx, float* a, float* b, float* kappa, float* phi, float* w, int B,
                             int H, int A, int U, int E, int att_type, float eps, float alignment,
                             float sharpening, float timing, void* stream) { PH_ENTRY();
    return gmm_attention_fwd_impl(h1, WattT, batt, kappa_prev, ctx, a, b, kappa, phi, w, B, H, A, U, E, att_type, eps, alignment,
                                  sharpening, timing, nullptr, stream);
}

int parrot_gmm_attention_fwd_sup(const float* h1, const float* WattT, const float* batt, const float* kappa_prev,
                                 const float* ctx, float* a, float* b, float* kappa, float* phi, float* w, int B,
                                 int H, int A, int U, int E, int att_type, float eps, float alignment,
                                 float sharpening, float timing, int* sup, void* stream) { PH_ENTRY();
    if (!sup) return PARROT_ERR_BADARG;
    return gmm_attention_fwd_impl(h1, WattT, batt, kappa_prev, ctx, a, b, kappa, phi, w, B, H, A, U, E, att_type, eps, alignment,
                                  sharpening, timing, sup, stream);
}

static int gmm_attention_bwd_impl(const float* dw, const float* ctx, const float* a, const float* b,
                                  const float* kappa, const float* kappa_prev, const float* WattT, float* dkappa,
                                  float* dp, float* dh1, int B, int H, int A, int U, int E, int att_type, float eps,
                                  const int* sup, void* stream) {
    if (!dw || !ctx || !a || !b || !kappa || !kappa_prev || !WattT || !dkappa || !dp || !dh1)
        return PARROT_ERR_BADARG;
    AttBwdArgs g{};
    g.sup = sup;
    g.dw = const_cast<float*>(dw); g.dw2 = nullptr; g.lddw = E; g.ctx = ctx; g.a = a; g.b = b; g.kappa = kappa; g.kappa_prev = kappa_prev;
    g.WattT = WattT; g.dkappa = dkappa; g.dp_out = dp; g.dh1 = dh1; g.lddh = H;
    g.B = B; g.H = H; g.A = A; g.U = U; g.E = E; g.att_type = att_type; g.eps = eps;
    return att_bwd_launch(g, (hipStream_t)stream);
}

int parrot_gmm_attention_bwd(const float* dw, const float* ctx, const float* a, const float* b,
                             const float* kappa, const float* kappa_prev, const float* WattT, float* dkappa,
                             float* dp, float* dh1, int B, int H, int A, int U, int E, int att_type, float eps,
                             void* stream) { PH_ENTRY();
    return gmm_attention_bwd_impl(dw, ctx, a, b, kappa, kappa_prev, WattT, dkappa, dp, dh1, B, H, A, U, E, att_type, eps,
                                  nullptr, stream);
}

int parrot_gmm_attention_bwd_sup(const float* dw, const float* ctx, const float* a, const float* b,
                                 const float* kappa, const float* kappa_prev, const float* WattT, float* dkappa,
                                 float* dp, float* dh1, int B, int H, int A, int U, int E, int att_type, float eps,
                                 const int* sup, void* stream) { PH_ENTRY();
    return gmm_attention_bwd_impl(dw, ctx, a, b, kappa, kappa_prev, WattT, dkappa, dp, dh1, B, H, A, U, E, att_type, eps, sup,
                                  stream);
}

int parrot_att_bwd_route(int U, int E, int has_sup, int u_lo, int u_hi, int* route) {
    // (no HIP call here: the query works without a device)
    if (!route || U < 1 || E < 1) return PARROT_ERR_BADARG;
    *route = att_bwd_route(sw_att_bwd_narrow(), has_sup != 0, U, E, u_lo, u_hi);
    return 0;
}

int parrot_sumsq(const float* x, size_t n, float* out, void* stream) { PH_ENTRY();
    return sumsq_launch(x, n, out, (hipStream_t)stream);
}

int parrot_adam_clip_step(float* param, const float* grad, float* m, float* v, size_t n,
                          const float* gnorm_sq, float grad_scale, float clip_threshold, float lr,
                          float beta1, float beta2, float eps, int step, void* stream) { PH_ENTRY();
    if (!param || !grad || !m || !v || step < 1) return PARROT_ERR_BADARG;
    if (clip_threshold > 0.f && !gnorm_sq) return PARROT_ERR_BADARG;
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, step)) / (1.0 - pow((double)beta1, step));
    return adam_clip_launch(param, grad, m, v, n, gnorm_sq, grad_scale, clip_threshold, (float)lr_t, beta1,
                            beta2, eps, (hipStream_t)stream);
}

int parrot_batch_quantize(const float* x, int rows, int n, int ld, double* ws, void* out, int ldo, int mode,
                          int q_levels, void* stream) { PH_ENTRY();
    if (!x || !ws || !out) return PARROT_ERR_BADARG;
    return quantize_launch(x, rows, n, ld, ws, out, ldo, mode, q_levels, (hipStream_t)stream);
}

int parrot_mu2linear(const int32_t* q, size_t n, float* out, void* stream) { PH_ENTRY();
    if (!q || !out) return PARROT_ERR_BADARG;
    return mu2linear_launch(q, n, out, (hipStream_t)stream);
}

}  // extern "C"

// Label tables of the text encoder (gfx950): what replaces the products with the embedded text.
//
// The encoder's input rows are rows of a small table: x2 = embed_label.W[labels], [Te Be, D] with Q = 43 distinct rows.
// So the fork products x2 . W are rows of the table P = embed_label.W . W + b ([Q, cols], one small product), and
// backward x2^T . dY = embed_label.W^T . S with S[q] = sum over the rows with label q of dY[row] ([Q, cols]); the bias
// gradient is sum_q S[q], and d embed_label.W = sum S . W^T.  x2, dx and the scatter into the table's gradient disappear
// (model.py _encoder_forward / _encoder_backward; the SampleRNN embedding has worked this way since trainops.hip).
//
//  * parrot_label_gather:  rows[s][i, :] = tbl[s][labels[i], :] for up to four tables in one launch (candidate and gate
//    inputs of both directions);
//  * parrot_label_segsum:  sums[s][q, :] = sum over i with labels[i] == q of rows[s][i, :], up to four matrices in one pair
//    of launches.  Small Q: no sort.  Pass 1, workgroup = (slice of LT_RPS rows, 64 columns of the concatenated column
//    space): lane = column, the two waves deal the slice's rows (wave w takes rows w, w + 2, ... in order) and add each
//    into its OWN [Q][64] table in LDS; the tables are added in wave order into ws[slice][q][column].  Pass 2 adds the
//    slices in slice order.  The order of the addends depends on (N, labels) alone: no float atomics, same bits every run.
//    Tables, partial sums and the slice sum are doubles, rounded to f32 once at the end, so a sum costs one f32 rounding:
//    the bias gradients are nothing but these sums, and they are held to the error of the column sums they replace.
#include <stdlib.h>

#include "../../include/parrot_hip.h"
#include "common.h"

namespace {

constexpr int LT_MAXQ = 64;     // LT_WAVES x Q x 64 doubles of LDS: 64 KB
constexpr int LT_WAVES = 2, LT_THREADS = 64 * LT_WAVES;
constexpr int LT_RPS = 128;     // rows of a slice

struct LtArgs {
    const int* labels;
    const float* tbl[4];
    float* rows[4];
    float* sums[4];
    int D[4], c0[5];  // columns of segment s, its first column in the concatenated space (c0[nseg] = total)
    long long N;
    int Q, nseg;
};

// thread = one 16-byte column group of one row of the concatenated column space
__global__ __launch_bounds__(256) void lt_gather_kernel(const LtArgs a) {
    const int G = a.c0[a.nseg] >> 2;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.N * G) return;
    const long long i = e / G;
    const int col = 4 * (int)(e % G);
    const int q = min(max(a.labels[i], 0), a.Q - 1);  // (bounds are the caller's to check; never read outside the table)
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (s < a.nseg && col >= a.c0[s] && col < a.c0[s + 1]) {
            const int c = col - a.c0[s];
            *reinterpret_cast<f32x4*>(a.rows[s] + (size_t)i * a.D[s] + c) =
                *reinterpret_cast<const f32x4*>(a.tbl[s] + (size_t)q * a.D[s] + c);
        }
}

// lane's column of the concatenated space -> (source pointer of row 0, row pitch); null past the last column
__device__ __forceinline__ const float* lt_column(const LtArgs& a, int col, int& pitch) {
    const float* p = nullptr;
    pitch = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (s < a.nseg && col >= a.c0[s] && col < a.c0[s + 1]) {
            p = a.rows[s] + (col - a.c0[s]);
            pitch = a.D[s];
        }
    return p;
}

__global__ __launch_bounds__(LT_THREADS) void lt_segsum_slice_kernel(const LtArgs a, double* __restrict__ ws) {
    extern __shared__ double tab[];  // [LT_WAVES][Q][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Q = a.Q, Dt = a.c0[a.nseg];
    const int col = blockIdx.y * 64 + lane;
    double* mine = tab + (size_t)wave * Q * 64;
    for (int q = 0; q < Q; ++q) mine[q * 64 + lane] = 0.0;
    int pitch;
    const float* src = lt_column(a, col, pitch);
    const long long r0 = (long long)blockIdx.x * LT_RPS, r1 = min(a.N, r0 + LT_RPS);
    if (src) {
        long long r = r0 + wave;
        for (; r + 3 * LT_WAVES < r1; r += 4 * LT_WAVES) {  // four rows in flight, added in row order
            float v[4];
            int q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = src[(size_t)(r + LT_WAVES * u) * pitch];
                q[u] = min(max(a.labels[r + LT_WAVES * u], 0), Q - 1);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) mine[q[u] * 64 + lane] += (double)v[u];
        }
        for (; r < r1; r += LT_WAVES) mine[min(max(a.labels[r], 0), Q - 1) * 64 + lane] += (double)src[(size_t)r * pitch];
    }
    __syncthreads();
    if (col < Dt)
        for (int q = wave; q < Q; q += LT_WAVES) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < LT_WAVES; ++w) t += tab[((size_t)w * Q + q) * 64 + lane];
            ws[((size_t)blockIdx.x * Q + q) * Dt + col] = t;
        }
}

// grid (Q, column blocks of 256)
__global__ __launch_bounds__(256) void lt_segsum_reduce_kernel(const LtArgs a, const double* __restrict__ ws, int nslices) {
    const int Q = a.Q, Dt = a.c0[a.nseg];
    const int q = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    if (col >= Dt) return;
    const double* p = ws + (size_t)q * Dt + col;
    const size_t step = (size_t)Q * Dt;
    double acc = 0.0;
    int sl = 0;
    for (; sl + 8 <= nslices; sl += 8) {  // eight slices in flight, added in slice order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(sl + u) * step];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; sl < nslices; ++sl) acc += p[(size_t)sl * step];
    const float out = (float)acc;  // the one rounding of a sum
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (s < a.nseg && col >= a.c0[s] && col < a.c0[s + 1]) a.sums[s][(size_t)q * a.D[s] + (col - a.c0[s])] = out;
}

int lt_args(const ParrotLabelTablesDesc* d, bool gather, LtArgs& a) {
    if (!d || !d->labels || d->N < 1 || d->Q < 1 || d->nseg < 1 || d->nseg > 4) return PH_ERR_BADARG;
    if (d->Q > LT_MAXQ) return PH_ERR_UNSUPPORTED;
    a.labels = d->labels; a.N = d->N; a.Q = d->Q; a.nseg = d->nseg;
    a.c0[0] = 0;
    for (int s = 0; s < 4; ++s) {
        a.tbl[s] = nullptr; a.rows[s] = nullptr; a.sums[s] = nullptr; a.D[s] = 0;
        if (s >= d->nseg) { a.c0[s + 1] = a.c0[s]; continue; }
        if (d->D[s] < 4 || (d->D[s] & 3) || !d->rows[s] || !(gather ? (const void*)d->tbl[s] : (const void*)d->sums[s]))
            return PH_ERR_BADARG;
        if (((uintptr_t)d->rows[s] & 15) || (gather && ((uintptr_t)d->tbl[s] & 15))) return PH_ERR_BADARG;
        a.tbl[s] = d->tbl[s]; a.rows[s] = d->rows[s]; a.sums[s] = d->sums[s]; a.D[s] = d->D[s];
        a.c0[s + 1] = a.c0[s] + d->D[s];
    }
    return 0;
}

}  // namespace

extern "C" {

int parrot_label_tables_supported(long long N, int Q) { return N >= 1 && Q >= 1 && Q <= LT_MAXQ; }

int parrot_label_gather(const ParrotLabelTablesDesc* desc, void* stream) { PH_ENTRY();
    LtArgs a;
    const int rc = lt_args(desc, true, a);
    if (rc) return rc;
    const long long blocks = (a.N * (a.c0[a.nseg] >> 2) + 255) / 256;
    if (blocks > 0x7fffffffll) return PH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lt_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

long long parrot_label_segsum_ws_floats(long long N, int Q, int Dtotal) { PH_ENTRY();
    if (N < 1 || Q < 1 || Dtotal < 1) return 0;
    return 2 * ((N + LT_RPS - 1) / LT_RPS) * Q * Dtotal;  // (doubles)
}

int parrot_label_segsum(const ParrotLabelTablesDesc* desc, float* ws, long long ws_floats, void* stream) { PH_ENTRY();
    LtArgs a;
    const int rc = lt_args(desc, false, a);
    if (rc) return rc;
    const int Dt = a.c0[a.nseg];
    if (!ws || ((uintptr_t)ws & 7) || ws_floats < parrot_label_segsum_ws_floats(a.N, a.Q, Dt)) return PH_ERR_BADARG;
    const long long nslices = (a.N + LT_RPS - 1) / LT_RPS;
    if (nslices > 0x7fffffffll) return PH_ERR_UNSUPPORTED;
    double* wsd = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(lt_segsum_slice_kernel, dim3((unsigned)nslices, (unsigned)ceil_div(Dt, 64)), dim3(LT_THREADS),
                       sizeof(double) * LT_WAVES * a.Q * 64, (hipStream_t)stream, a, wsd);
    PH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lt_segsum_reduce_kernel, dim3((unsigned)a.Q, (unsigned)ceil_div(Dt, 256)), dim3(256), 0,
                       (hipStream_t)stream, a, wsd, (int)nslices);
    return (int)hipGetLastError();
}

}  // extern "C"

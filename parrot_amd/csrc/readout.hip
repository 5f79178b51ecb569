// Training: the readout stack and the output layer as ONE affine map of rank <= 64 (include/parrot_hip.h,
// ParrotReadoutComposedDesc).  pred = X . W' + b' with W' = Wr . Wo: products of width 64 that stream X = [h_0 | .. | w]
// once, instead of three products of width R through a [T*B, R] readouts buffer and back.
//
// Kernels (all f32 operands, f32 accumulation on v_mfma_f32_16x16x4_f32; operand lane maps as skinny.hip: lane
// (kk = l >> 4, i = l & 15) holds A[row i][k = 4 kk + u] and B[k = 4 kk + u][col i] for the step u of a 16-deep chunk,
// C/D col = l & 15, row = 4 (l >> 4) + reg):
//   ro_compose_kernel    W' and b' in double, rounded once; W' is written as two fragment-major copies:
//                        Wf[((c16 * 4 + n) * 64 + lane) * 4 + u] = W'[16 c16 + 4 kk + u][16 n + i]     (forward: B = W')
//                        Wb[((c16 * 4 + q) * 64 + lane) * 4 + u] = W'[16 c16 + i][16 q + 4 kk + u]     (data backward: B = W'^T)
//                        so that 64 K rows of either are one contiguous 16 KB block whose lanes read 16-byte vectors.
//   ro_fwd_kernel        pred = b' + sum_s x_s . W'_s: 128 rows of M per workgroup, W' walked in 64-row blocks through LDS,
//                        four partial sums along K added pairwise.
//   ro_bwd_data_kernel   dx_s = dp . W'_s^T: the [32, 64] dp tile of a wave stays in registers, W' walked as above.
//   ro_bwd_w_kernel      partial dW' = x^T . dp per slice of M, plus the column sums of dp as one more row
//   ro_reduce_kernel     dW' = the slices' tiles added in slice order (in double, rounded once)
//   ro_gwr_kernel, ro_gwo_part_kernel, ro_gwo_finish_kernel, ro_bias_grads_kernel
//                        the decomposition into the factors' gradients: gWr += dW' . Wo^T, gWo += Wr^T . dW' + rbsum (x) sum dp
//                        and the bias gradients, 0.3 GFLOP in all, accumulated in double and rounded once into the gradient
//                        (like the composition itself: what the composed path adds to the M-long sums is one rounding each).
// No float atomics, no scratch.
#include "common.h"
#include "readout.h"

namespace {

struct RoSegs {
    const float* x[PARROT_READOUT_MAX_SEG];
    float* dx[PARROT_READOUT_MAX_SEG];   // first data row (below the zero rows)
    int K[PARROT_READOUT_MAX_SEG];
    int ldx[PARROT_READOUT_MAX_SEG];
    int lddx[PARROT_READOUT_MAX_SEG];
    int nseg, Ktot;
};

struct RoBias {
    const float* rb[PARROT_READOUT_MAX_SEG];
    float* grb[PARROT_READOUT_MAX_SEG];
    int n;
};

// ---------------------------------------------------------------------------------------------- compose
// Blocks 0 .. Ktot/8 - 1: eight rows of W' each (thread = one column, two rows); the last block: rbsum and b'.
__global__ __launch_bounds__(256) void ro_compose_kernel(const float* __restrict__ Wr, int ldwr, const float* __restrict__ Wo,
                                                         int ldwo, int R, int O, int Ktot, RoBias bias,
                                                         const float* __restrict__ bo, float* __restrict__ Wf,
                                                         float* __restrict__ Wb, float* __restrict__ bp,
                                                         float* __restrict__ rbsum) {
    __shared__ float sWr[8][64];
    __shared__ float sWo[64][64];
    __shared__ double sred[4][64];
    const int t = threadIdx.x, o = t & 63, q = t >> 6;
    if ((int)blockIdx.x == Ktot / 8) {
        double acc = 0.0;
        for (int r = q; r < R; r += 4) {
            double s = 0.0;
            for (int i = 0; i < bias.n; ++i) s += (double)bias.rb[i][r];
            if (o == 0) rbsum[r] = (float)s;
            if (o < O) acc += s * (double)Wo[(size_t)r * ldwo + o];
        }
        sred[q][o] = acc;
        __syncthreads();
        if (q == 0) {
            const double v = ((sred[0][o] + sred[1][o]) + (sred[2][o] + sred[3][o])) + (o < O ? (double)bo[o] : 0.0);
            bp[o] = o < O ? (float)v : 0.f;
        }
        return;
    }
    const int k0 = blockIdx.x * 8;
    double acc0 = 0.0, acc1 = 0.0;
    for (int r0 = 0; r0 < R; r0 += 64) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = t + 256 * u, i = e >> 6, rr = e & 63;
            sWr[i][rr] = (r0 + rr < R) ? Wr[(size_t)(k0 + i) * ldwr + r0 + rr] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int rr = q + 4 * u;
            sWo[rr][o] = (r0 + rr < R && o < O) ? Wo[(size_t)(r0 + rr) * ldwo + o] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int rr = 0; rr < 64; ++rr) {
            const double w = (double)sWo[rr][o];
            acc0 += (double)sWr[q][rr] * w;
            acc1 += (double)sWr[q + 4][rr] * w;
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int k = k0 + q + 4 * u;
        const float v = (float)(u ? acc1 : acc0);
        const int c16 = k >> 4, kin = k & 15;
        Wf[(((size_t)c16 * 4 + (o >> 4)) * 64 + ((kin >> 2) * 16 + (o & 15))) * 4 + (kin & 3)] = v;
        Wb[(((size_t)c16 * 4 + (o >> 4)) * 64 + ((((o & 15) >> 2)) * 16 + kin)) * 4 + (o & 3)] = v;
    }
}

// 64 K rows (4096 floats) of a fragment-major copy, global -> registers -> LDS, by a workgroup of 1024 / NV threads.
template <int NV>
__device__ __forceinline__ void ro_stage_load(const float* __restrict__ W, int g, int Ktot, f32x4 (&r)[NV]) {
    const size_t lim = (size_t)Ktot * RO_NP;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const size_t e = (size_t)g * 4096 + (size_t)(threadIdx.x + (1024 / NV) * u) * 4;
        r[u] = e < lim ? *reinterpret_cast<const f32x4*>(W + e) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
template <int NV>
__device__ __forceinline__ void ro_stage_store(float* s, const f32x4 (&r)[NV]) {
#pragma unroll
    for (int u = 0; u < NV; ++u) *reinterpret_cast<f32x4*>(s + (threadIdx.x + (1024 / NV) * u) * 4) = r[u];
}

// Segment and offset inside it of global K row k (a multiple of 16: never straddles a segment).
__device__ __forceinline__ void ro_seg_of(const RoSegs& s, int k, int& si, int& kb) {
    si = 0;
    kb = k;
#pragma unroll
    for (int i = 0; i < PARROT_READOUT_MAX_SEG - 1; ++i)
        if (si == i && i + 1 < s.nseg && kb >= s.K[i]) { kb -= s.K[i]; si = i + 1; }
}

// ---------------------------------------------------------------------------------------------- forward
// 512 threads: eight waves of 16 rows.  The K reduction runs on FOUR accumulator sets (one per 16-deep chunk of a 64-row
// block) added pairwise at the end: a quarter of the chain length of one running sum, half its rounding error.
__global__ __launch_bounds__(512) void ro_fwd_kernel(const RoSegs s, int M, int O, const float* __restrict__ Wf,
                                                     const float* __restrict__ bp, float* __restrict__ pred, int ldp) {
    __shared__ __attribute__((aligned(16))) float sW[2][4096];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kk = lane >> 4, ci = lane & 15;
    const int m0 = blockIdx.x * RO_MROWS + wave * 16;
    const bool mok = m0 + ci < M;
    const int mrow = mok ? m0 + ci : M - 1;
    f32x4 acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[q][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nc16 = s.Ktot >> 4, ngroups = (nc16 + 3) >> 2;
    f32x4 st[2];
    ro_stage_load<2>(Wf, 0, s.Ktot, st);
    ro_stage_store<2>(sW[0], st);
    __syncthreads();
    for (int g = 0; g < ngroups; ++g) {
        const int cur = g & 1;
        if (g + 1 < ngroups) ro_stage_load<2>(Wf, g + 1, s.Ktot, st);
        f32x4 a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c16 = g * 4 + q;
            if (c16 < nc16) {
                int si, kb;
                ro_seg_of(s, c16 * 16, si, kb);
                a[q] = *reinterpret_cast<const f32x4*>(s.x[si] + kb + 4 * kk + (size_t)mrow * s.ldx[si]);
                if (!mok) a[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (g * 4 + q < nc16) {
                f32x4 b[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) b[n] = *reinterpret_cast<const f32x4*>(&sW[cur][((q * 4 + n) * 64 + lane) * 4]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        acc[q][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][u], b[n][u], acc[q][n], 0, 0, 0);
            }
        }
        if (g + 1 < ngroups) ro_stage_store<2>(sW[cur ^ 1], st);
        __syncthreads();
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int col = 16 * n + ci;
        if (col >= O) continue;
        const float bias = bp[col];
        const f32x4 v = (acc[0][n] + acc[1][n]) + (acc[2][n] + acc[3][n]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + kk * 4 + j;
            if (m < M) pred[(size_t)m * ldp + col] = v[j] + bias;
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward, data
// Blocks 0 .. nmb - 1: 128 rows of M each; the RO_ZERO_BLOCKS blocks behind them zero-fill the rows above the data rows.
__global__ __launch_bounds__(256) void ro_bwd_data_kernel(const RoSegs s, int M, int O, int nmb, int zero_rows,
                                                          const float* __restrict__ Wb, const float* __restrict__ dp,
                                                          int lddp) {
    __shared__ __attribute__((aligned(16))) float sW[2][4096];
    if ((int)blockIdx.x >= nmb) {
        const int zb = blockIdx.x - nmb;
        for (int si = 0; si < s.nseg; ++si) {
            const int K = s.K[si], ld = s.lddx[si];
            float* top = s.dx[si] - (size_t)zero_rows * ld;
            const long long total = (long long)zero_rows * K;
            for (long long e = (long long)zb * 256 + threadIdx.x; e < total; e += (long long)RO_ZERO_BLOCKS * 256)
                top[(size_t)(e / K) * ld + (int)(e % K)] = 0.f;
        }
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kk = lane >> 4, ci = lane & 15;
    const int m0 = blockIdx.x * RO_MROWS + wave * 32;
    // the wave's dp tile as the A operand: reduction index o = 16 q + 4 kk + u
    f32x4 ad[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = m0 + mt * 16 + ci;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int o = 16 * q + 4 * kk + u;
                ad[mt][q][u] = (m < M && o < O) ? dp[(size_t)m * lddp + o] : 0.f;
            }
    }
    const int nc16 = s.Ktot >> 4, ngroups = (nc16 + 3) >> 2;
    f32x4 st[4];
    ro_stage_load<4>(Wb, 0, s.Ktot, st);
    ro_stage_store<4>(sW[0], st);
    __syncthreads();
    for (int g = 0; g < ngroups; ++g) {
        const int cur = g & 1;
        if (g + 1 < ngroups) ro_stage_load<4>(Wb, g + 1, s.Ktot, st);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int c16 = g * 4 + q4;
            if (c16 < nc16) {
                f32x4 b[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) b[q] = *reinterpret_cast<const f32x4*>(&sW[cur][((q4 * 4 + q) * 64 + lane) * 4]);
                // one accumulator per 16 output columns of the reduction, added pairwise: chains of 16, not 64
                f32x4 pa[2][4];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int q = 0; q < 4; ++q) pa[mt][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt)
                            pa[mt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[mt][q][u], b[q][u], pa[mt][q], 0, 0, 0);
                const f32x4 acc[2] = {(pa[0][0] + pa[0][1]) + (pa[0][2] + pa[0][3]), (pa[1][0] + pa[1][1]) + (pa[1][2] + pa[1][3])};
                int si, kb;
                ro_seg_of(s, c16 * 16, si, kb);
                float* out = s.dx[si] + kb + ci;
                const int ld = s.lddx[si];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int m = m0 + mt * 16 + kk * 4 + j;
                        if (m < M) out[(size_t)m * ld] = acc[mt][j];
                    }
            }
        }
        if (g + 1 < ngroups) ro_stage_store<4>(sW[cur ^ 1], st);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- backward, weights
// grid (kgroups, nslice).  Wave w of block (bx, slice) owns the 64 rows k0 = (4 bx + w) * 64 .. + 63 of dW' for the
// slice's rows of M.  A operand = x^T: lane (r = l & 15, kq = l >> 4) loads x[m + kq][k0 + 4 r .. + 3] (a row of x is read
// as whole 256-byte runs) and uses element u for the accumulators of the row set {k0 + 4 r' + u}; B operand = dp rows
// m + kq from an LDS image in fragment order, sD[((step * 64 + lane) * 4) + n] = dp[m = 4 step + kq][16 n + i].
// Wave 0 of the bx = 0 blocks also multiplies a row of ones: the column sums of dp, stored as row Ktot.
__global__ __launch_bounds__(256) void ro_bwd_w_kernel(const RoSegs s, int M, int O, int slice_rows,
                                                       const float* __restrict__ dp, int lddp, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sD[4096];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, ci = lane & 15;
    const int k0 = (blockIdx.x * 4 + wave) * RO_KSTRIP;
    const int slice = blockIdx.y;
    const int mbeg = slice * slice_rows;
    const int mend = min(M, mbeg + slice_rows);
    const bool wave_on = k0 < s.Ktot;
    const bool do_sum = blockIdx.x == 0 && wave == 0;
    // this lane's four K rows: k0 + 4 ci .. + 3 (inside one segment: segment bounds are multiples of 16)
    const int kl = k0 + 4 * ci;
    const bool lane_on = kl < s.Ktot;
    const float* xp = s.x[0];
    int ld = s.ldx[0];
    {
        int kb = lane_on ? kl : 0;
        bool found = false;
#pragma unroll
        for (int i = 0; i < PARROT_READOUT_MAX_SEG; ++i) {
            if (i < s.nseg && !found) {
                if (kb < s.K[i]) { xp = s.x[i] + kb; ld = s.ldx[i]; found = true; }
                else kb -= s.K[i];
            }
        }
    }
    f32x4 acc[4][4];
    f32x4 accs[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        accs[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[u][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float sr[16];
    auto stage_load = [&](int mb) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = threadIdx.x + 256 * u, ml = e >> 6, o = e & 63;
            const int m = mb + ml;
            sr[u] = (m < mend && o < O) ? dp[(size_t)m * lddp + o] : 0.f;
        }
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = threadIdx.x + 256 * u, ml = e >> 6, o = e & 63;
            sD[(((ml >> 2) * 64 + (ml & 3) * 16 + (o & 15)) * 4) + (o >> 4)] = sr[u];
        }
    };
    stage_load(mbeg);
    for (int mb = mbeg; mb < mend; mb += RO_MCHUNK) {
        __syncthreads();   // the previous chunk's reads are done
        stage_store();
        __syncthreads();
        if (mb + RO_MCHUNK < mend) stage_load(mb + RO_MCHUNK);
        if (wave_on) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 xa[8];
#pragma unroll
                for (int t8 = 0; t8 < 8; ++t8) {
                    const int m = mb + 4 * (half * 8 + t8) + kq;
                    xa[t8] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (lane_on && m < mend) xa[t8] = *reinterpret_cast<const f32x4*>(xp + (size_t)m * ld);
                }
#pragma unroll
                for (int t8 = 0; t8 < 8; ++t8) {
                    const int step = half * 8 + t8;
                    const f32x4 b = *reinterpret_cast<const f32x4*>(&sD[(step * 64 + lane) * 4]);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int n = 0; n < 4; ++n)
                            acc[u][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[t8][u], b[n], acc[u][n], 0, 0, 0);
                    if (do_sum) {
#pragma unroll
                        for (int n = 0; n < 4; ++n)
                            accs[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, b[n], accs[n], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (!wave_on) return;
    float* pt = part + (size_t)slice * ((size_t)s.Ktot + 1) * RO_NP;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 4 * (kq * 4 + j) + u;
                if (k < s.Ktot) pt[(size_t)k * RO_NP + 16 * n + ci] = acc[u][n][j];
            }
    if (do_sum && kq == 0) {
#pragma unroll
        for (int n = 0; n < 4; ++n) pt[(size_t)s.Ktot * RO_NP + 16 * n + ci] = accs[n][0];
    }
}

// dW'[i] = sum of the slices' partial tiles, in slice order, in double.  n4 = float4 elements per tile.
__global__ __launch_bounds__(256) void ro_reduce_kernel(const f32x4* __restrict__ part, f32x4* __restrict__ dW, int n4,
                                                        int nslice) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    int sl = 0;
    for (; sl + 8 <= nslice; sl += 8) {
        f32x4 p[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) p[q] = part[(size_t)(sl + q) * n4 + i];
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] += (double)p[q][u];
    }
    for (; sl < nslice; ++sl) {
        const f32x4 p = part[(size_t)sl * n4 + i];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] += (double)p[u];
    }
    dW[i] = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// gWr[k, r] += sum_o dW'[k, o] Wo[r, o].  grid (ceil(R / 64), Ktot / 16); thread = one r, four k.
__global__ __launch_bounds__(256) void ro_gwr_kernel(const float* __restrict__ dW, const float* __restrict__ Wo, int ldwo,
                                                     int R, int O, float* __restrict__ gWr, int ldgwr) {
    __shared__ float sD[16][64];
    __shared__ float sWo[64][65];
    const int t = threadIdx.x, rl = t & 63, kq = t >> 6;
    const int r0 = blockIdx.x * 64, k0 = blockIdx.y * 16;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = t + 256 * u;
        sD[e >> 6][e & 63] = dW[(size_t)(k0 + (e >> 6)) * RO_NP + (e & 63)];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = t + 256 * u, rr = e >> 6, o = e & 63;
        sWo[rr][o] = (r0 + rr < R && o < O) ? Wo[(size_t)(r0 + rr) * ldwo + o] : 0.f;
    }
    __syncthreads();
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (int o = 0; o < 64; ++o) {
        const double w = (double)sWo[rl][o];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += (double)sD[kq * 4 + i][o] * w;
    }
    const int r = r0 + rl;
    if (r >= R) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float* g = gWr + (size_t)(k0 + kq * 4 + i) * ldgwr + r;
        *g = (float)((double)*g + acc[i]);
    }
}

// part[ks][r][o] = sum over the K rows [ks * 128, + 128) of Wr[k, r] dW'[k, o].  grid (ceil(R / 64), slices);
// thread = one o, sixteen r.
__global__ __launch_bounds__(256) void ro_gwo_part_kernel(const float* __restrict__ Wr, int ldwr, const float* __restrict__ dW,
                                                          int R, int Ktot, double* __restrict__ part) {
    __shared__ float sWr[16][64];
    __shared__ float sD[16][64];
    const int t = threadIdx.x, o = t & 63, rq = t >> 6;
    const int r0 = blockIdx.x * 64, kbeg = blockIdx.y * RO_GWO_KROWS, kend = min(Ktot, kbeg + RO_GWO_KROWS);
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0;
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = t + 256 * u, i = e >> 6, c = e & 63;
            sWr[i][c] = (r0 + c < R) ? Wr[(size_t)(k0 + i) * ldwr + r0 + c] : 0.f;
            sD[i][c] = dW[(size_t)(k0 + i) * RO_NP + c];
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const double d = (double)sD[i][o];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] += (double)sWr[i][rq * 16 + j] * d;
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int r = r0 + rq * 16 + j;
        if (r < R) part[((size_t)blockIdx.y * R + r) * RO_NP + o] = acc[j];
    }
}

// gWo[r, o] += the slices' tiles in slice order + rbsum[r] * sdp[o]; one thread per (r, o of 64).
__global__ __launch_bounds__(256) void ro_gwo_finish_kernel(const double* __restrict__ part, int nks, int R, int O,
                                                            const float* __restrict__ rbsum, const float* __restrict__ sdp,
                                                            float* __restrict__ gWo, int ldgwo) {
    const int e = blockIdx.x * 256 + threadIdx.x, r = e >> 6, o = e & 63;
    if (r >= R || o >= O) return;
    double v = (double)rbsum[r] * (double)sdp[o];
    for (int ks = 0; ks < nks; ++ks) v += part[((size_t)ks * R + r) * RO_NP + o];
    float* g = gWo + (size_t)r * ldgwo + o;
    *g = (float)((double)*g + v);
}

// sdp = column sums of dp (row Ktot of dW').  Thread r: t = sdp . Wo[r, :] -> every readout bias gradient; block 0 also
// gbo += sdp.
__global__ __launch_bounds__(256) void ro_bias_grads_kernel(const float* __restrict__ sdp, const float* __restrict__ Wo,
                                                            int ldwo, int R, int O, float* __restrict__ gbo, RoBias bias) {
    __shared__ float ss[RO_NP];
    if (threadIdx.x < RO_NP) ss[threadIdx.x] = sdp[threadIdx.x];
    __syncthreads();
    if (blockIdx.x == 0 && (int)threadIdx.x < O) gbo[threadIdx.x] += ss[threadIdx.x];
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    double t = 0.0;
    for (int o = 0; o < O; ++o) t += (double)ss[o] * (double)Wo[(size_t)r * ldwo + o];
    for (int i = 0; i < bias.n; ++i) bias.grb[i][r] = (float)((double)bias.grb[i][r] + t);
}

RoSegs ro_segs(const ParrotReadoutComposedDesc* d, int Ktot, bool bwd) {
    RoSegs s{};
    s.nseg = d->nseg;
    s.Ktot = Ktot;
    for (int i = 0; i < d->nseg; ++i) {
        s.x[i] = d->x[i];
        s.K[i] = d->K[i];
        s.ldx[i] = d->ldx[i];
        s.lddx[i] = d->lddx[i];
        s.dx[i] = bwd ? d->dx[i] + (size_t)d->zero_rows * d->lddx[i] : nullptr;
    }
    return s;
}

int ro_prepare(const ParrotReadoutComposedDesc* d, const float* ws, RoLayout& L) {
    int rc = ro_layout(d, &L);
    if (rc) return rc;
    rc = ro_check_operands(d);
    if (rc) return rc;
    if (!ws || ((uintptr_t)ws & 15) || d->ws_floats < L.total) return PARROT_ERR_BADARG;
    return 0;
}

}  // namespace

extern "C" {

long long parrot_readout_composed_ws_floats(const ParrotReadoutComposedDesc* desc) { PH_ENTRY();
    RoLayout L;
    const int rc = ro_layout(desc, &L);
    return rc ? -(long long)rc : L.total;
}

int parrot_readout_composed_fwd(const ParrotReadoutComposedDesc* d, float* ws, void* stream) { PH_ENTRY();
    RoLayout L;
    int rc = ro_prepare(d, ws, L);
    if (rc) return rc;
    if (!d->pred || d->ldp < d->O) return PARROT_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    RoBias b{};
    b.n = d->nbias;
    for (int i = 0; i < d->nbias; ++i) b.rb[i] = d->rb[i];
    hipLaunchKernelGGL(ro_compose_kernel, dim3(L.Ktot / 8 + 1), dim3(256), 0, st, d->Wr, d->ldwr, d->Wo, d->ldwo, d->R, d->O,
                       L.Ktot, b, d->bo, ws + L.Wf, ws + L.Wb, ws + L.bp, ws + L.rbsum);
    PH_CHECK(hipGetLastError());
    const RoSegs s = ro_segs(d, L.Ktot, false);
    const int nmb = (int)((d->M + RO_MROWS - 1) / RO_MROWS);
    hipLaunchKernelGGL(ro_fwd_kernel, dim3(nmb), dim3(512), 0, st, s, (int)d->M, d->O, ws + L.Wf, ws + L.bp, d->pred, d->ldp);
    return (int)hipGetLastError();
}

int parrot_readout_composed_bwd(const ParrotReadoutComposedDesc* d, float* ws, void* stream) { PH_ENTRY();
    RoLayout L;
    int rc = ro_prepare(d, ws, L);
    if (rc) return rc;
    if (!d->dp || d->lddp < d->O || !d->gWr || !d->gWo || !d->gbo || d->ldgwr < d->R || d->ldgwo < d->O) return PARROT_ERR_BADARG;
    for (int i = 0; i < d->nseg; ++i)
        if (!d->dx[i] || d->lddx[i] < d->K[i]) return PARROT_ERR_BADARG;
    for (int i = 0; i < d->nbias; ++i)
        if (!d->grb[i]) return PARROT_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const RoSegs s = ro_segs(d, L.Ktot, true);
    const int M = (int)d->M;
    const int nmb = (M + RO_MROWS - 1) / RO_MROWS;
    hipLaunchKernelGGL(ro_bwd_data_kernel, dim3(nmb + RO_ZERO_BLOCKS), dim3(256), 0, st, s, M, d->O, nmb, d->zero_rows,
                       ws + L.Wb, d->dp, d->lddp);
    PH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ro_bwd_w_kernel, dim3(L.kgroups, L.nslice), dim3(256), 0, st, s, M, d->O, L.slice_rows, d->dp, d->lddp,
                       ws + L.part);
    PH_CHECK(hipGetLastError());
    const int n4 = (L.Ktot + 1) * (RO_NP / 4);
    hipLaunchKernelGGL(ro_reduce_kernel, dim3((n4 + 255) / 256), dim3(256), 0, st, reinterpret_cast<const f32x4*>(ws + L.part),
                       reinterpret_cast<f32x4*>(ws + L.dW), n4, L.nslice);
    PH_CHECK(hipGetLastError());
    const float* dW = ws + L.dW;
    const float* sdp = dW + (size_t)L.Ktot * RO_NP;
    hipLaunchKernelGGL(ro_gwr_kernel, dim3((d->R + 63) / 64, L.Ktot / 16), dim3(256), 0, st, dW, d->Wo, d->ldwo, d->R, d->O,
                       d->gWr, d->ldgwr);
    PH_CHECK(hipGetLastError());
    double* gpart = reinterpret_cast<double*>(ws + L.gwo);
    hipLaunchKernelGGL(ro_gwo_part_kernel, dim3((d->R + 63) / 64, L.gwo_slices), dim3(256), 0, st, d->Wr, d->ldwr, dW, d->R,
                       L.Ktot, gpart);
    PH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ro_gwo_finish_kernel, dim3((d->R * RO_NP + 255) / 256), dim3(256), 0, st, gpart, L.gwo_slices, d->R, d->O,
                       ws + L.rbsum, sdp, d->gWo, d->ldgwo);
    PH_CHECK(hipGetLastError());
    RoBias b{};
    b.n = d->nbias;
    for (int i = 0; i < d->nbias; ++i) { b.rb[i] = d->rb[i]; b.grb[i] = d->grb[i]; }
    hipLaunchKernelGGL(ro_bias_grads_kernel, dim3((d->R + 255) / 256), dim3(256), 0, st, sdp, d->Wo, d->ldwo, d->R, d->O,
                       d->gbo, b);
    return (int)hipGetLastError();
}

}  // extern "C"

// Mixture-density head of the training step (gfx950): the Gaussian-mixture negative log-likelihood of model.py:65-91 on
// the pre-activations of the three output heads (model.py:774-781), and its gradient, one pass over the rows each way.
//
//   sig_ok = exp(sig_hat_ok) + eps                pi_k = softmax(co_hat)_k + eps
//   a_k    = log pi_k - 1/2 sum_o [ (y_o - mu_ok)^2 / sig_ok^2 + 2 log sig_ok + log 2 pi ]
//   nll    = -( log sum_k exp(a_k - max a) + max a )          logr_k = a_k + nll   (log responsibility)
//
//   d nll / d mu_ok      = - r_k (y_o - mu_ok) / sig_ok^2                              r_k = exp(logr_k)
//   d nll / d sig_hat_ok =   r_k (1 / sig_ok - (y_o - mu_ok)^2 / sig_ok^3) exp(sig_hat_ok)
//   d nll / d co_hat_j   =   p_j (q_j - sum_k p_k q_k)          p = softmax(co_hat),  q_k = - r_k / pi_k
//
// Mapping: one wave per row, four rows per workgroup.  A row of mu / sig_hat is O groups of K components (column o*K + k).
// With G = 64 / K, lane l < G*K reads element i*G*K + l in iteration i: one contiguous run per load, k = l mod K fixed per
// lane, o = i*G + l / K.  GC_U iterations' loads (mu and sig_hat interleaved) are issued before the first use.  The G
// partial sums of a component are added in group order (__shfl), the K-wide max / sum / sum p q are fixed trees over the
// lanes below K: no atomics, no scratch, one order of summation -> the same bits every run.  The backward pass walks the
// row the same way and needs no second pass because logr is saved.
#include <math.h>

#include "../../include/parrot_hip.h"
#include "common.h"

namespace {

constexpr int GC_U = 4;                          // iterations in flight
constexpr float GC_HALF_LOG_2PI = 0.91893853320467274178f;

__device__ __forceinline__ float gc_wave_max(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
    return v;
}

// softmax over the K lanes below K (every lane passes the co_hat of ITS k = lane mod K; the lanes at and above K hold
// copies and stay out of the sums): exp(c - max) / sum, as torch.softmax computes it.
__device__ __forceinline__ float gc_softmax(float c, bool first) {
    const float cm = gc_wave_max(first ? c : -INFINITY);
    const float e = expf(c - cm);
    return e / wave_sum(first ? e : 0.f);
}

__global__ __launch_bounds__(256) void gmm_cost_fwd_kernel(const float* __restrict__ y, int ldy, const float* __restrict__ mu,
                                                           int ldmu, const float* __restrict__ sh, int ldsig,
                                                           const float* __restrict__ co, int ldco, long long M, int O, int K,
                                                           float eps, float* __restrict__ nll, float* __restrict__ pi_out,
                                                           int ldpi, float* __restrict__ logr) {
    const int lane = threadIdx.x & 63;
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;  // (wave-uniform)
    const int G = 64 / K, GK = G * K, n = O * K;
    const int k = lane % K, g = lane / K;
    const bool act = lane < GK, first = lane < K;
    const float* ym = y + m * ldy;
    const float* mum = mu + m * ldmu;
    const float* shm = sh + m * ldsig;
    const float c = co[m * ldco + k];

    float acc = 0.f;  // sum over this lane's o of  1/2 z^2 + log sig
    for (int base = 0, ob = g; base < n; base += GC_U * GK, ob += GC_U * G) {
        float vm[GC_U], vs[GC_U], vy[GC_U];
        bool ok[GC_U];
#pragma unroll
        for (int u = 0; u < GC_U; ++u) {
            const int idx = base + u * GK + lane;  // = (ob + u*G) * K + k, so idx < n  <=>  o < O
            ok[u] = act && idx < n;
            vm[u] = ok[u] ? mum[idx] : 0.f;
            vs[u] = ok[u] ? shm[idx] : 0.f;
            vy[u] = ok[u] ? ym[ob + u * G] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < GC_U; ++u) {
            const float s = expf(vs[u]) + eps;
            const float z = (vy[u] - vm[u]) * __builtin_amdgcn_rcpf(s);
            const float t = fmaf(0.5f * z, z, logf(s));
            acc += ok[u] ? t : 0.f;
        }
    }
    float tot = 0.f;  // the component's G partial sums in group order; every lane ends with the total of its k
    for (int gg = 0; gg < G; ++gg) tot += __shfl(acc, k + gg * K, 64);

    const float pi = gc_softmax(c, first) + eps;
    const float a = logf(pi) - tot - (float)O * GC_HALF_LOG_2PI;
    const float am = gc_wave_max(first ? a : -INFINITY);
    const float da = a - am;
    const float ls = logf(wave_sum(first ? expf(da) : 0.f));
    const float nl = -(ls + am);
    if (first) {
        // a_k + nll as (a_k - max a) - log sum: both terms small, so the rounding of nll (|nll| ~ 100 at O = 63: half an
        // ulp is 4e-6) does not become a relative error of every responsibility of the row
        logr[m * K + k] = da - ls;
        if (pi_out) pi_out[m * ldpi + k] = pi;
    }
    if (lane == 0) nll[m] = nl;
}

__global__ __launch_bounds__(256) void gmm_cost_bwd_kernel(const float* __restrict__ y, int ldy, const float* __restrict__ mu,
                                                           int ldmu, const float* __restrict__ sh, int ldsig,
                                                           const float* __restrict__ co, int ldco,
                                                           const float* __restrict__ logr, const float* __restrict__ rowscale,
                                                           long long M, int O, int K, float eps, float* __restrict__ dmu,
                                                           int lddmu, float* __restrict__ dsh, int lddsig,
                                                           float* __restrict__ dco, int lddco) {
    const int lane = threadIdx.x & 63;
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;  // (wave-uniform)
    const int G = 64 / K, GK = G * K, n = O * K;
    const int k = lane % K, g = lane / K;
    const bool act = lane < GK, first = lane < K;
    const float* ym = y + m * ldy;
    const float* mum = mu + m * ldmu;
    const float* shm = sh + m * ldsig;
    float* dmum = dmu + m * lddmu;
    float* dshm = dsh + m * lddsig;
    const float rs = rowscale[m];
    const float r = expf(logr[m * K + k]);
    const float rr = rs * r;

    const float p = gc_softmax(co[m * ldco + k], first);
    const float q = -r / (p + eps);
    const float spq = wave_sum(first ? p * q : 0.f);
    // a masked row (rowscale 0) stores 0.0 whatever its operands are: 0 * (z / sig) would be NaN once z / sig overflows
    const bool dead = rs == 0.f;
    if (first) dco[m * lddco + k] = dead ? 0.f : rs * (p * (q - spq));

    for (int base = 0, ob = g; base < n; base += GC_U * GK, ob += GC_U * G) {
        float vm[GC_U], vs[GC_U], vy[GC_U];
        bool ok[GC_U];
#pragma unroll
        for (int u = 0; u < GC_U; ++u) {
            const int idx = base + u * GK + lane;
            ok[u] = act && idx < n;
            vm[u] = ok[u] ? mum[idx] : 0.f;
            vs[u] = ok[u] ? shm[idx] : 0.f;
            vy[u] = ok[u] ? ym[ob + u * G] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < GC_U; ++u) {
            const int idx = base + u * GK + lane;
            const float e = expf(vs[u]);
            const float inv = __builtin_amdgcn_rcpf(e + eps);
            const float z = (vy[u] - vm[u]) * inv;  // (y - mu) / sig
            if (ok[u]) {
                dmum[idx] = dead ? 0.f : -rr * (z * inv);
                dshm[idx] = dead ? 0.f : rr * ((inv - z * z * inv) * e);
            }
        }
    }
}

bool gc_bad_common(const void* y, int ldy, const void* mu, int ldmu, const void* sh, int ldsig, const void* co, int ldco,
                   long long M, int O, int K) {
    if (!y || !mu || !sh || !co || M < 1 || O < 1 || K < 1) return true;
    const long long w = (long long)O * K;
    return ldy < O || ldmu < w || ldsig < w || ldco < K || w > 0x7fffffffll;
}

// [p, p + (M-1)*ld + width) floats: what a call touches of a row-major [M, width] operand
struct GcSpan { const float* lo; const float* hi; };
GcSpan gc_span(const float* p, long long M, long long ld, long long width) { return {p, p + (M - 1) * ld + width}; }
bool gc_overlap(const GcSpan& a, const GcSpan& b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" {

int parrot_gmm_cost_fwd(const float* y, int ldy, const float* mu, int ldmu, const float* sig_hat, int ldsig,
                        const float* co_hat, int ldco, long long M, int O, int K, float eps, float* nll, float* pi_out,
                        int ldpi, float* logr, void* stream) { PH_ENTRY();
    if (gc_bad_common(y, ldy, mu, ldmu, sig_hat, ldsig, co_hat, ldco, M, O, K) || !nll || !logr || (pi_out && ldpi < K))
        return PH_ERR_BADARG;
    const long long blocks = (M + 3) / 4;
    if (K > 64 || blocks > 0x7fffffffll) return PH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gmm_cost_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y, ldy, mu, ldmu,
                       sig_hat, ldsig, co_hat, ldco, M, O, K, eps, nll, pi_out, ldpi, logr);
    return (int)hipGetLastError();
}

int parrot_gmm_cost_bwd(const float* y, int ldy, const float* mu, int ldmu, const float* sig_hat, int ldsig,
                        const float* co_hat, int ldco, const float* logr, const float* rowscale, long long M, int O, int K,
                        float eps, float* dmu, int lddmu, float* dsig_hat, int lddsig, float* dco_hat, int lddco,
                        void* stream) { PH_ENTRY();
    if (gc_bad_common(y, ldy, mu, ldmu, sig_hat, ldsig, co_hat, ldco, M, O, K) || !logr || !rowscale || !dmu || !dsig_hat ||
        !dco_hat || lddmu < (long long)O * K || lddsig < (long long)O * K || lddco < K)
        return PH_ERR_BADARG;
    // the gradients may overlap neither an input (mu is handed back to the caller as next_x) nor each other
    const long long W = (long long)O * K;
    const GcSpan outs[3] = {gc_span(dmu, M, lddmu, W), gc_span(dsig_hat, M, lddsig, W), gc_span(dco_hat, M, lddco, K)};
    const GcSpan ins[6] = {gc_span(y, M, ldy, O), gc_span(mu, M, ldmu, W), gc_span(sig_hat, M, ldsig, W),
                           gc_span(co_hat, M, ldco, K), gc_span(logr, M, K, K), gc_span(rowscale, M, 1, 1)};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 6; ++j)
            if (gc_overlap(outs[i], ins[j])) return PH_ERR_BADARG;
        for (int j = i + 1; j < 3; ++j)
            if (gc_overlap(outs[i], outs[j])) return PH_ERR_BADARG;
    }
    const long long blocks = (M + 3) / 4;
    if (K > 64 || blocks > 0x7fffffffll) return PH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gmm_cost_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y, ldy, mu, ldmu,
                       sig_hat, ldsig, co_hat, ldco, logr, rowscale, M, O, K, eps, dmu, lddmu, dsig_hat, lddsig, dco_hat,
                       lddco);
    return (int)hipGetLastError();
}

}  // extern "C"

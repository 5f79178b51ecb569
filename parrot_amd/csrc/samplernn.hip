// Conditional three-tier SampleRNN generation loop on the device (gfx950).
//
// Replaces the per-sample Python loop of reference three_tier.py:809-832, which crosses the
// host/device boundary three times per audio sample (big_frame_level_generate_fn every 80 samples,
// frame_level_generate_fn every 10, sample_level_generate_fn every sample).  Here the whole loop is a
// fixed launch sequence per 80-sample period (1 big-tier step, 8 frame-tier steps, 80 sample-MLP
// steps) captured once into a hipGraph and replayed per period; the running sample index lives in
// device memory, so no value ever returns to the host inside the loop.
//
// Arithmetic restated from sampleRNN/lib/ops.py:329-393 (GRU step with the Input linear inside the
// step) and three_tier.py:291-515; weight norm (ops.py:101-110) is folded by the caller, and the
// sample-level Embedding (ops.py:252-266) is folded with SampleLevel.L1_PrevSamples into a
// [FS, Q, D] table, which turns the K = FS*EMB GEMM into a 10-row gather-sum.
#include <new>
#include <stdlib.h>

#include "../../include/parrot_hip.h"
#include "biggemm.h"
#include "skinny.h"
#include "sr_common.h"
#include "sr_persist.h"
#include "sr_stage.h"
#include "switches.h"

namespace {


// xf[b][i] = (s / (Q/2) - 1) * 2 for the `n` samples before t (three_tier.py:309-310, 398-399);
// optionally copies the conditioning frame of the current big frame.
__global__ __launch_bounds__(256) void sr_prep_kernel(const int* __restrict__ samples, int len, const int* __restrict__ tbase,
                                                      int toff, int n, float half_q, float* __restrict__ xf, int B,
                                                      const float* __restrict__ feats, float* __restrict__ feat_cur,
                                                      int feat_dim, int bfs) {
    const int t = tbase[0] + toff;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < B * n) {
        const int b = idx / n, i = idx % n;
        xf[idx] = ((float)samples[(size_t)b * len + t - n + i] / half_q - 1.0f) * 2.0f;
    }
    if (feats && idx < B * feat_dim) {
        const int b = idx / feat_dim, f = idx % feat_dim;
        feat_cur[idx] = feats[((size_t)(t / bfs) * B + b) * feat_dim + f];
    }
}

// o1[b][d] = sum_pos tbl[pos][samples[b][t-FS+pos]][d] + frame_out[b][d]   (frame_out row already offset)
__global__ __launch_bounds__(256) void sr_embed_sum_kernel(const int* __restrict__ samples, int len,
                                                           const int* __restrict__ tbase, int toff, int FS, int Q, int D,
                                                           const float* __restrict__ tbl, const float* __restrict__ frame_out,
                                                           int ldf, float* __restrict__ o1) {
    const int t = tbase[0] + toff;
    const int b = blockIdx.y;
    const int d4 = blockIdx.x * 256 + threadIdx.x;  // float4 index
    if (d4 * 4 >= D) return;
    f32x4 acc = *reinterpret_cast<const f32x4*>(frame_out + (size_t)b * ldf + d4 * 4);
    for (int pos = 0; pos < FS; ++pos) {
        const int q = samples[(size_t)b * len + t - FS + pos];
        acc += *reinterpret_cast<const f32x4*>(tbl + ((size_t)pos * Q + q) * D + d4 * 4);
    }
    *reinterpret_cast<f32x4*>(o1 + (size_t)b * D + d4 * 4) = acc;
}

// samples[b][t] = argmax_q logits[b][q] (lowest index on ties, like numpy / Theano argmax), or a
// temperature-scaled multinomial draw from a counter-based generator when temperature > 0 -- among all Q codes, or among
// the top_k most likely ones (SampleRnnGenDesc::top_k: terms 0.0f outside the kept set, same sums, same uniform), or among
// the nucleus of those (samplernn_generate_set_top_p: the shortest prefix of the same order with top_p of their mass), and of
// what both left the codes whose term is >= min_p (samplernn_generate_set_min_p).
// forced (samplernn_generate_set_forced, or null): where forced[b][t] is a code in 0 .. Q-1 it is the sample, whatever was
// picked; any other value leaves the pick.  logp (samplernn_generate_set_log_probs, or null): logp[b][t] = the natural
// logarithm of softmax(logits)[sample] at temperature 1, without truncation.  Both through emit(), which every branch
// ends in; both for any Q.  dlogp / kept (samplernn_generate_set_draw_stats, or both null): what the step drew from -- the
// size of the kept set (1 on an argmax step, Q untruncated) and the log of the sample's probability under the draw's own
// temperature and kept set (-inf outside it).  Through emit() where the set is all codes or the argmax (any Q), through
// stats() by wave 0 behind a truncated draw (Q <= 256): the kept terms' mass is srp_wave_sum's fixed tree.
__global__ __launch_bounds__(256) void sr_pick_kernel(const float* __restrict__ logits, int Q, int* __restrict__ samples,
                                                      int len, const int* __restrict__ tbase, int toff, float temperature,
                                                      unsigned long long seed, const unsigned long long* __restrict__ origin,
                                                      const SrUttDraw* __restrict__ utt, int draw_mode, int top_k,
                                                      float top_p, float min_p, const int* __restrict__ forced,
                                                      float* __restrict__ logp, float* __restrict__ dlogp,
                                                      int* __restrict__ kept) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ float se[256];
    const int t = tbase[0] + toff;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* lg = logits + (size_t)b * Q;
    // (a value that is no code never indexes anything: it means "free")
    const int fv = forced ? forced[(size_t)b * len + t] : -1;
    const bool is_forced = (unsigned)fv < (unsigned)Q;
    float lse = 0.f;  // log sum_q exp(logits[q] - max), with logp only
    float dlse = 0.f;  // log sum_q exp((logits[q] - max) / temperature), with dlogp on an untruncated draw only
    bool full = true;  // the step draws among all codes or takes the argmax: emit() writes the statistics
    auto emit = [&](int pick) {
        const int s = is_forced ? fv : pick;
        samples[(size_t)b * len + t] = s;
        if (logp) logp[(size_t)b * len + t] = lg[s] - sv[0] - lse;
        if (dlogp && full) {
            const bool greedy = temperature <= 0.f;
            dlogp[(size_t)b * len + t] = greedy ? (s == si[0] ? 0.f : -INFINITY) : (lg[s] - sv[0]) / temperature - dlse;
            kept[(size_t)b * len + t] = greedy ? 1 : Q;
        }
    };
    // the statistics of a truncated draw, by all of wave 0 behind it: lane `lane` holds n <= 4 codes code(j) with kept bits
    // keep, `pick` is lane 0's
    auto stats = [&](unsigned keep, int n, int pick, auto code) {
        if (!dlogp) return;
        const int s = __builtin_amdgcn_readfirstlane(is_forced ? fv : pick);
        float m = 0.f;
        int cnt = 0;
        bool in = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool k = j < n && ((keep >> j) & 1u);
            const float e = k ? expf((lg[min(code(j), Q - 1)] - sv[0]) / temperature) : 0.f;
            m = j == 0 ? e : __fadd_rn(m, e);
            cnt += (int)__popcll(__ballot(k));
            in = in || (k && code(j) == s);
        }
        const float tot = srp_wave_sum(m);
        const bool any = __ballot(in) != 0ull;
        if (threadIdx.x == 0) {
            dlogp[(size_t)b * len + t] = any ? (lg[s] - sv[0]) / temperature - logf(tot) : -INFINITY;
            kept[(size_t)b * len + t] = cnt;
        }
    };
    // key = what the draw's counter is hashed with: the plan's seed and the stream, or (per-utterance entries, a uniform
    // branch) the utterance's seed alone, with its own temperature and its counter taken back by the run index of its prefix
    unsigned long long key = seed ^ (0xBF58476D1CE4E5B9ull * (unsigned long long)(b + 1)), off = 0;
    if (utt) { key = utt[b].seed; off = utt[b].off; temperature = utt[b].temperature; top_k = utt[b].top_k; top_p = utt[b].top_p; min_p = utt[b].min_p; }
    // top-k truncation (a uniform branch of both draws; create admits it for Q <= 256 only): wave 0 selects the kept set with
    // the persistent kernel's helper, four codes per lane at most; off, a draw runs the instructions it always ran
    top_k = __builtin_amdgcn_readfirstlane(top_k);
    const bool use_k = top_k > 0 && top_k < Q && Q <= 256;
    // the nucleus, behind top-k when both are active (the setters admit it for Q <= 256 only): srp_topp_keep, same lanes
    top_p = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(top_p)));
    const bool use_p = top_p > 0.f && top_p < 1.f && Q <= 256;
    // min-p, behind both (Q <= 256 only, like them): srp_minp_keep on the same lanes' terms
    min_p = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(min_p)));
    const bool use_m = min_p > 0.f && min_p <= 1.f && Q <= 256;
    const bool trunc = use_k || use_p || use_m;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int q = tid; q < Q; q += 256) {
        const float v = lg[q];
        if (v > best || (v == best && q < bi)) { best = v; bi = q; }
    }
    sv[tid] = best; si[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const float v = sv[tid + s];
            const int i = si[tid + s];
            if (v > sv[tid] || (v == sv[tid] && i < si[tid])) { sv[tid] = v; si[tid] = i; }
        }
        __syncthreads();
    }
    if (logp) {  // (a uniform branch) the block's fixed tree over the threads' partial sums
        const float mx = sv[0];
        float e = 0.f;
        for (int q = tid; q < Q; q += 256) e += expf(lg[q] - mx);
        se[tid] = e;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) se[tid] += se[tid + s];
            __syncthreads();
        }
        lse = logf(se[0]);
    }
    if (temperature <= 0.f) {
        if (tid == 0) emit(si[0]);
        return;
    }
    full = !trunc;
    if (dlogp && full) {  // (a uniform branch) the mass of all codes at the draw's temperature, the same fixed tree
        __syncthreads();  // (se may still be read for lse)
        const float mx = sv[0];
        float e = 0.f;
        for (int q = tid; q < Q; q += 256) e += expf((lg[q] - mx) / temperature);
        se[tid] = e;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) se[tid] += se[tid + s];
            __syncthreads();
        }
        dlse = logf(se[0]);
    }
    if (draw_mode == 1) {
        // wave-parallel draw (a uniform branch; create has checked that Q is a multiple of 64): wave 0, lane l owns the
        // Q / 64 contiguous codes from l Q / 64 on; same terms, key, counter and uniform as the walk below
        if (tid < 64) {
            const float mx = sv[0];
            const int n = Q / 64;
            const float u01 = srp_u01(key, origin[0] + (unsigned long long)(t + 1) - off);
            int pick;
            if (trunc) {  // (n <= 4) the terms outside the kept set are 0.0f, the fall-through picks the highest kept code
                unsigned f[4];
                int idx[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { idx[j] = n * tid + j; f[j] = j < n ? srp_order_image(lg[min(idx[j], Q - 1)]) : 0u; }
                unsigned keep = use_k ? srp_topk_keep<4>(f, idx, top_k) : (1u << n) - 1u;
                if (use_p) {
                    float ek[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) ek[j] = (keep >> j) & 1u ? expf((lg[min(idx[j], Q - 1)] - mx) / temperature) : 0.f;
                    keep &= srp_topp_keep<4>(f, idx, ek, top_p);
                }
                if (use_m) {
                    float ek[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) ek[j] = (keep >> j) & 1u ? expf((lg[min(idx[j], Q - 1)] - mx) / temperature) : 0.f;
                    keep &= srp_minp_keep<4>(ek, min_p);
                }
                const int lk = keep ? n * tid + 31 - __clz((int)keep) : -1;
                pick = srp_scan_draw<true>([&](int j) { return (keep >> j) & 1u ? expf((lg[n * tid + j] - mx) / temperature) : 0.f; },
                                           n, tid, u01, lk);
                if (tid == 0) emit(pick);
                stats(keep, n, pick, [&](int j) { return n * tid + j; });
                return;
            } else {
                pick = srp_scan_draw([&](int j) { return expf((lg[n * tid + j] - mx) / temperature); }, n, tid, u01);
            }
            if (tid == 0) emit(pick);
        }
        return;
    }
    if (trunc) {
        // the sequential walk among the kept codes: wave 0 selects (lane l holds codes l + 64 m) and leaves the kept flags
        // in si; thread 0 walks all Q codes in today's order with 0.0f for the others (adding it is exact)
        if (tid < 64) {
            unsigned f[4];
            int idx[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) { idx[m] = tid + 64 * m; f[m] = idx[m] < Q ? srp_order_image(lg[idx[m]]) : 0u; }
            unsigned keep = 0;
#pragma unroll
            for (int m = 0; m < 4; ++m) keep |= idx[m] < Q ? 1u << m : 0u;
            if (use_k) keep = srp_topk_keep<4>(f, idx, top_k);
            if (use_p) {
                float ek[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) ek[m] = (keep >> m) & 1u ? expf((lg[min(idx[m], Q - 1)] - sv[0]) / temperature) : 0.f;
                keep &= srp_topp_keep<4>(f, idx, ek, top_p);
            }
            if (use_m) {
                float ek[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) ek[m] = (keep >> m) & 1u ? expf((lg[min(idx[m], Q - 1)] - sv[0]) / temperature) : 0.f;
                keep &= srp_minp_keep<4>(ek, min_p);
            }
            const int last = srp_topk_last<4>(keep, idx);
#pragma unroll
            for (int m = 0; m < 4; ++m) si[idx[m]] = (int)((keep >> m) & 1u);
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            int pick = last;
            if (tid == 0) {
                const float mx = sv[0];
                float tot = 0.f;
                for (int q = 0; q < Q; ++q) tot += si[q] ? expf((lg[q] - mx) / temperature) : 0.f;
                const float u = srp_u01(key, origin[0] + (unsigned long long)(t + 1) - off) * tot;
                float c = 0.f;
                for (int q = 0; q < Q; ++q) {
                    c += si[q] ? expf((lg[q] - mx) / temperature) : 0.f;
                    if (u < c) { pick = q; break; }
                }
                emit(pick);
            }
            stats(keep, 4, pick, [&](int m) { return tid + 64 * m; });
        }
        return;
    }
    // inverse-CDF sampling of softmax(logits / temperature) by one thread (Q = 256)
    if (tid == 0) {
        const float mx = sv[0];
        float tot = 0.f;
        for (int q = 0; q < Q; ++q) tot += expf((lg[q] - mx) / temperature);
        // (keyed by the sample's index in the whole run: the draw origin counts what resumed segments have moved past)
        const float u = srp_u01(key, origin[0] + (unsigned long long)(t + 1) - off) * tot;
        float c = 0.f;
        int pick = Q - 1;
        for (int q = 0; q < Q; ++q) {
            c += expf((lg[q] - mx) / temperature);
            if (u < c) { pick = q; break; }
        }
        emit(pick);
    }
}

// Frame-tier input (three_tier.py:398-411): out[b][d] = bias[d] + add[b][d] + sum_i xf(b, i) * Win[i][d] with
// xf = (sample / (Q/2) - 1) * 2 of the FS samples before t: the K = FS product is ten FMAs per output, taken
// straight from the integer samples.
__global__ __launch_bounds__(256) void sr_frame_in_kernel(const int* __restrict__ samples, int len, const int* __restrict__ tbase,
                                                          int toff, int FS, float half_q, const float* __restrict__ Win,
                                                          const float* __restrict__ bias, const float* __restrict__ add,
                                                          int ld_add, float* __restrict__ out, int D,
                                                          const float* __restrict__ gpre = nullptr, const float* __restrict__ h = nullptr,
                                                          float* __restrict__ z = nullptr, float* __restrict__ rh = nullptr, int Dh = 0) {
    const int t = tbase[0] + toff;
    const int b = blockIdx.y, dd = blockIdx.x * 256 + threadIdx.x;
    if (dd >= D) return;
    float acc = 0.f;
    for (int i = 0; i < FS; ++i) {
        const float xf = ((float)samples[(size_t)b * len + t - FS + i] / half_q - 1.0f) * 2.0f;
        acc = fmaf(xf, Win[(size_t)i * D + dd], acc);
    }
    acc += (bias ? bias[dd] : 0.f) + add[(size_t)b * ld_add + dd];
    if (gpre && dd < 2 * Dh) {
        // (D = 3 Dh: gates | candidate) the recurrent product h . Wg of this frame's gates is there already (the previous
        // frame's projection launch made it): the gates are finished here, as the sample kernel's tail does for the frames
        // inside a period -- the frame costs one launch less
        const float gt = ph_sigmoid(gpre[(size_t)b * 2 * Dh + dd] + acc);
        if (dd < Dh) z[(size_t)b * Dh + dd] = gt;
        else rh[(size_t)b * Dh + dd - Dh] = gt * h[(size_t)b * Dh + dd - Dh];
        return;
    }
    out[(size_t)b * D + dd] = acc;
}

// (origin: the draw origin, set to 0 with tbase in front of a run that does not resume; null inside a period)
__global__ void sr_tick_kernel(int* tbase, int inc, int set, unsigned long long* origin) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        tbase[0] = set ? inc : tbase[0] + inc;
        if (set && origin) origin[0] = 0;
    }
}

// Per-utterance draws at the start of a run that does not resume: every stream's first utterance has its prefix in slot 0,
// so entry b = (row 1 of the caller's arrays, off 0).  Outside the period graphs, beside the sr_tick_kernel call that sets
// tbase; a start flagged at frame 1 then rewrites the same values.
__global__ __launch_bounds__(256) void sr_utt_init_kernel(SrUttDraw* __restrict__ utt, const unsigned long long* __restrict__ seed1,
                                                          const float* __restrict__ temp1, const int* __restrict__ top_k1,
                                                          int top_k, const float* __restrict__ top_p1, float top_p,
                                                          const float* __restrict__ min_p1, float min_p, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    utt[b].seed = seed1[b];
    utt[b].off = 0;
    utt[b].temperature = temp1[b];
    utt[b].top_k = top_k1 ? top_k1[b] : top_k;  // (no array of the caller's: the plan's)
    utt[b].top_p = top_p1 ? top_p1[b] : top_p;
    utt[b].min_p = min_p1 ? min_p1[b] : min_p;
}

// Segment boundary of a resumed run (samplernn_generate_run_segment, resume = 1): the first launch of the segment, outside
// the period graphs.  The plan's buffer is a ring of T slots: the last slot the previous run wrote, tbase / BFS - 1 whatever
// its length was, becomes slot 0 of every stream (the only history a period reads), tbase goes back to BFS, and the draw
// origin moves on by the samples the ring has turned past, so that a seeded draw stays keyed by the sample's index in the
// whole run.  The sample kernel's carry holds that slot's last samples and their table sums, keyed by the sample index
// they were left for: the blocks with the key of the old tbase are re-keyed to BFS (the next launch takes them as it
// does inside a run), any other block is invalidated.  The per-utterance draw entries stay as they are: their `off` is a
// run index, and origin + t does not change when the ring turns.  One workgroup: every thread has read tbase before it is rewritten.
struct SrResumeArgs {
    int* tbase; int* samples; unsigned long long* origin;
    int B, T, BFS, len;
    SrpCarryKeys carry;  // (key0 null: no persistent kernel)
};

__global__ __launch_bounds__(256) void sr_resume_kernel(const SrResumeArgs a) {
    const int tid = threadIdx.x;
    const int tb = a.tbase[0], last = tb / a.BFS - 1;
    __syncthreads();
    if (last < 1 || last >= a.T) return;  // (nothing has run: the host refuses that before it gets here)
    for (int idx = tid; idx < a.B * a.BFS; idx += 256) {
        const int b = idx / a.BFS, i = idx % a.BFS;
        a.samples[(size_t)b * a.len + i] = a.samples[(size_t)b * a.len + (size_t)last * a.BFS + i];
    }
    if (a.carry.key0)
        for (int k = tid; k < a.carry.blocks; k += 256) {
            int* key = a.carry.key0 + (size_t)k * a.carry.stride;
            key[0] = key[0] == tb ? a.BFS : -1;
        }
    if (tid == 0) {
        a.tbase[0] = a.BFS;
        a.origin[0] += (unsigned long long)last * (unsigned long long)a.BFS;
    }
}

// Utterance starts inside a packed run (SampleRnnGenDesc::starts): the first launch of a period.  Block b looks at
// starts[f][b], f = the big frame this period generates; a flagged stream gets what the first period of a run of its own
// finds -- slot f - 1 = Q/2 (all three levels read their history from `samples`), every state that outlives a period =
// the learned h0, its row of the next frame's gate product = h0 . Wg (the copy run() kept), and the carry of its team
// invalidated (the other rows of the team then read their true history from `samples` too).  With per-utterance draws
// the stream's entry becomes (utt_seed[f][b], run index of the prefix slot = origin + (f - 1) BFS, utt_temp[f][b],
// utt_top_k[f][b] or the plan's top_k, utt_top_p[f][b] or the plan's top_p, utt_min_p[f][b] or the plan's min_p).  Rows without a flag are not touched.
struct SrStartArgs {
    const int* starts; const int* tbase;
    int* samples;
    int B, D, T, BFS, len, q0;
    int nstate;                  // row states [B][D] to reset: state[i][b][:] = h0[i][:]
    float* state[20]; const float* h0[20];
    float* gpre; const float* gpre0;  // [B][2D] both (null: no such product on this path)
    SrpCarryKeys carry;
    SrUttDraw* utt;                   // [B] per-utterance draw entries (null: none)
    const unsigned long long* utt_seed; const float* utt_temp;  // [T][B] both, indexed like starts
    const unsigned long long* origin;
    const int* utt_top_k; int top_k;  // [T][B] like utt_temp, or null: every utterance takes the plan's top_k
    const float* utt_top_p; float top_p;  // likewise (samplernn_generate_set_utterance_top_p, samplernn_generate_set_top_p)
    const float* utt_min_p; float min_p;  // likewise (samplernn_generate_set_utterance_min_p, samplernn_generate_set_min_p)
};

__global__ __launch_bounds__(256) void sr_start_kernel(const SrStartArgs a) {
    const int f = a.tbase[0] / a.BFS, b = blockIdx.x, tid = threadIdx.x;
    if (f < 1 || f >= a.T || b >= a.B || a.starts[(size_t)f * a.B + b] == 0) return;
    for (int i = tid; i < a.BFS; i += 256) a.samples[(size_t)b * a.len + (size_t)(f - 1) * a.BFS + i] = a.q0;
    for (int s = 0; s < a.nstate; ++s)
        for (int i = tid; i < a.D; i += 256) a.state[s][(size_t)b * a.D + i] = a.h0[s][i];
    if (a.gpre)
        for (int i = tid; i < 2 * a.D; i += 256) a.gpre[(size_t)b * 2 * a.D + i] = a.gpre0[(size_t)b * 2 * a.D + i];
    if (a.carry.key0 && tid == 0) srp_carry_invalidate(a.carry, b);
    if (a.utt && tid == 0) {
        a.utt[b].seed = a.utt_seed[(size_t)f * a.B + b];
        a.utt[b].off = a.origin[0] + (unsigned long long)(f - 1) * (unsigned long long)a.BFS;
        a.utt[b].temperature = a.utt_temp[(size_t)f * a.B + b];
        a.utt[b].top_k = a.utt_top_k ? a.utt_top_k[(size_t)f * a.B + b] : a.top_k;
        a.utt[b].top_p = a.utt_top_p ? a.utt_top_p[(size_t)f * a.B + b] : a.top_p;
        a.utt[b].min_p = a.utt_min_p ? a.utt_min_p[(size_t)f * a.B + b] : a.min_p;
    }
}

#define SR_TRY(x)                 \
    do {                          \
        const int rc__ = (x);     \
        if (rc__ != 0) return rc__; \
    } while (0)

struct SrPlan {
    SampleRnnGenDesc d;
    bool persist = false;  // sample steps on the persistent-thread kernel (sr_persist.hip)
    int groups = 0;        // ... in this many row groups of 32 streams per launch (0: not persistent)
    // Fragment-major copies (sk_tile_weights, mode 0) of the single-GRU tiers' matrices, owned by the plan and made once
    // at create time: the step kernel then reads its weights as contiguous 1 KB wave loads instead of 64-byte row pieces.
    struct Tiled { float* U = nullptr; float* Wg = nullptr; float* Wc = nullptr; float* Wout = nullptr; };
    Tiled t_big, t_frm;
    float* tiled_slab = nullptr;
    // Persistent sample kernel (round 5): everything in front of L2's ReLU is linear, so it is composed through W2 once --
    //   t2tbl[pos] = emb_tbl[pos] . W2  [FS, Q, D],   Pout_i = Wout_i . W2  [D, FS*D],   cb_i = bout_i . W2 + b2  [FS*D]
    // -- the frame tier's projection launch makes h . Pout + cb (same shape and cost as h . Wout + bout) and the sample
    // kernel's L2 pre-activation is a gather-sum: one product and one hand-off fewer per audio sample.
    float* t2tbl = nullptr; float* Pout = nullptr; float* cb = nullptr;
    // Round 5 (single-GRU tiers): the frame tier's input xf . Win + bin + big_out only enters the step through x . U, so
    //   x . U + bU = xf . (Win . U) + [(bin + big_out) . U + bU].
    // winu = Win . U [FS, 3D] and pbias = bin . U + bU [3D] are composed once (the weights are fixed for the plan's life);
    // per 80-sample period ONE product makes pbig[b][f] = big_out[b, f] . U + pbias for all BFS / FS frames, and the two step
    // GEMMs of a frame walk K = D (their own recurrent product) instead of 2 D, with pin [B, 3D] = xf . winu + pbig[f] as
    // their additive input -- written by the previous frame's sample kernel (SrpArgs::next_n) or, for the first frame of a
    // period, by sr_frame_in_kernel at width 3D.
    float* winu = nullptr; float* pbias = nullptr; float* pbig = nullptr; float* pin = nullptr;
    float* gpre = nullptr;  // [B, 2D] h . Wg of the next frame, made beside the projection (persistent path)
    // Packed runs (d.starts): what run() leaves in gpre in front of the first period, h0 . Wg of every row, kept outside the
    // period graph.  sr_start_kernel copies row b of it when stream b begins an utterance: the bits a run of that utterance
    // in the same stream starts from, whatever tile of that launch the row was in.
    float* gpre0 = nullptr;
    // Draw origin (one device word, owned by the plan): samples the resumed segments of the current run have moved past;
    // the seeded draw of buffer index t is keyed by origin + t.  A device word because the periods replay from graphs.
    unsigned long long* origin = nullptr;
    bool has_run = false;  // a run has been issued: resume = 1 has something to continue
    // Per-utterance draws (samplernn_generate_set_utterance_draws): [B] entries owned by the plan, allocated by the setter
    // (outside stream capture, like origin), and the caller's [T][B] arrays.  Null: the plan's key and temperature.
    SrUttDraw* utt = nullptr;
    const unsigned long long* utt_seed = nullptr;
    const float* utt_temp = nullptr;
    int set_utt(const unsigned long long* seed, const float* temp) {
        if (!utt) {
            if (hipMalloc(&utt, (size_t)d.B * sizeof(SrUttDraw)) != hipSuccess) { utt = nullptr; return (int)hipErrorOutOfMemory; }
            PH_CHECK(hipMemset(utt, 0, (size_t)d.B * sizeof(SrUttDraw)));
        }
        utt_seed = seed; utt_temp = temp;
        return 0;
    }
    // samplernn_generate_set_utterance_top_k: the caller's [T][B] truncations beside them (null: the plan's top_k for all)
    const int* utt_top_k = nullptr;
    // samplernn_generate_set_top_p / _set_utterance_top_p: the plan's nucleus (0: off; the descriptor has no word for it) and
    // the caller's [T][B] values (null: the plan's for all)
    float top_p = 0.f;
    const float* utt_top_p = nullptr;
    // samplernn_generate_set_min_p / _set_utterance_min_p: likewise the plan's min_p (0: off) and the caller's [T][B] values
    float min_p = 0.f;
    const float* utt_min_p = nullptr;
    // samplernn_generate_set_forced / _set_log_probs: the caller's [B][BFS * T] arrays, indexed like d.samples (null: off).
    // Indexed by buffer index, so a resumed segment needs no state of theirs: the host stages them per segment, like features.
    const int* forced = nullptr;
    float* logp = nullptr;
    // samplernn_generate_set_draw_stats: likewise, both or neither
    float* dlogp = nullptr;
    int* kept = nullptr;
    // samplernn_generate_set_skip_stacks: Graves' stacks (ops.py:650-695, 861-880).  Layer k >= 1 reads [h_{k-1} ; x] through
    // its [2D, N] Input matrix (slot 0 of big_L[k] / frm_L[k]) and the tier's output is sum_k h_k . S_k + bS.
    SampleRnnSkipStacks skip{};
    bool has_skip = false;
    int make_origin() {
        if (hipMalloc(&origin, sizeof(unsigned long long)) != hipSuccess) { origin = nullptr; return 1; }
        return (int)hipMemset(origin, 0, sizeof(unsigned long long));
    }
    int make_winu() {
        const size_t D = d.D, nfr = d.BFS / d.FS;
        if (d.n_rnn != 0) return 0;
        if (hipMalloc(&winu, ((size_t)d.FS * 3 * D + 3 * D + (size_t)d.B * nfr * 3 * D + (size_t)d.B * 3 * D + (size_t)d.B * 2 * D + (d.starts ? (size_t)d.B * 2 * D : 0)) * sizeof(float)) != hipSuccess) {
            winu = nullptr;
            return 0;
        }
        pbias = winu + (size_t)d.FS * 3 * D;
        pbig = pbias + 3 * D;
        pin = pbig + (size_t)d.B * nfr * 3 * D;
        gpre = pin + (size_t)d.B * 3 * D;
        if (d.starts) gpre0 = gpre + (size_t)d.B * 2 * D;
        BgPrecisionScope f32_only(0);
        int rc = parrot_gemm(d.frm_Win, (int)D, 0, d.frm_U, 3 * (int)D, 0, winu, 3 * (int)D, d.FS, 3 * (int)D, (int)D, nullptr, 1.f, 0, 0,
                             1, 0, 0, 0, 1, nullptr);
        if (rc == 0)
            rc = parrot_gemm(d.frm_bin, (int)D, 0, d.frm_U, 3 * (int)D, 0, pbias, 3 * (int)D, 1, 3 * (int)D, (int)D, d.frm_bU, 1.f, 0, 0,
                             1, 0, 0, 0, 1, nullptr);
        if (rc == 0) rc = (int)hipDeviceSynchronize();
        if (rc != 0) { (void)hipFree(winu); winu = nullptr; gpre0 = nullptr; }
        return 0;
    }
    int make_composed() {
        const size_t D = d.D, Q = d.Q, FS = d.FS;
        if (hipMalloc(&t2tbl, (FS * Q * D + D * FS * D + FS * D) * sizeof(float)) != hipSuccess) { t2tbl = nullptr; return 1; }
        Pout = t2tbl + FS * Q * D;
        cb = Pout + D * FS * D;
        BgPrecisionScope f32_only(0);  // whatever the process-wide GEMM precision is: these tables feed an f32 path
        int rc = parrot_gemm(d.emb_tbl, (int)D, 0, d.W2, (int)D, 0, t2tbl, (int)D, (int)(FS * Q), (int)D, (int)D, nullptr, 1.f, 0, 0, 1,
                             0, 0, 0, 1, nullptr);
        for (size_t i = 0; i < FS && rc == 0; ++i) {
            rc = parrot_gemm(d.frm_Wout + i * D, (int)(FS * D), 0, d.W2, (int)D, 0, Pout + i * D, (int)(FS * D), (int)D, (int)D, (int)D,
                             nullptr, 1.f, 0, 0, 1, 0, 0, 0, 1, nullptr);
            if (rc == 0)
                rc = parrot_gemm(d.frm_bout + i * D, (int)D, 0, d.W2, (int)D, 0, cb + i * D, (int)D, 1, (int)D, (int)D, d.b2, 1.f, 0, 0,
                                 1, 0, 0, 0, 1, nullptr);
        }
        if (rc == 0) rc = (int)hipDeviceSynchronize();
        if (rc != 0) { (void)hipFree(t2tbl); t2tbl = nullptr; Pout = cb = nullptr; }
        return rc;
    }
    int make_tiled() {
        const size_t D = d.D, nfr = d.BFS / d.FS;
        if (d.n_rnn != 0 || (d.D & 15)) return 0;
        const size_t per = 3 * D * D + 2 * D * D + D * D;
        const size_t total = 2 * per + D * nfr * D + D * d.FS * D;
        if (hipMalloc(&tiled_slab, total * sizeof(float)) != hipSuccess) { tiled_slab = nullptr; return 0; }
        float* p = tiled_slab;
        auto tile = [&](const float* W, int rows, int cols, float*& dst) -> int {
            dst = p;
            p += (size_t)rows * cols;
            return sk_tile_weights_launch(W, rows, cols, cols, dst, 0, 0, nullptr);
        };
        int rc = 0;
        rc |= tile(d.big_U, d.D, 3 * d.D, t_big.U); rc |= tile(d.big_Wg, d.D, 2 * d.D, t_big.Wg);
        rc |= tile(d.big_Wc, d.D, d.D, t_big.Wc); rc |= tile(d.big_Wout, d.D, (int)nfr * d.D, t_big.Wout);
        rc |= tile(d.frm_U, d.D, 3 * d.D, t_frm.U); rc |= tile(d.frm_Wg, d.D, 2 * d.D, t_frm.Wg);
        rc |= tile(d.frm_Wc, d.D, d.D, t_frm.Wc); rc |= tile(persist ? Pout : d.frm_Wout, d.D, d.FS * d.D, t_frm.Wout);
        if (rc != 0 || hipDeviceSynchronize() != hipSuccess) {
            (void)hipFree(tiled_slab);
            tiled_slab = nullptr;
            t_big = Tiled(); t_frm = Tiled();
        }
        return 0;
    }
    enum { SR_CHUNK = 8 };
    hipGraphExec_t exec = nullptr, exec_chunk = nullptr;
    int periods_left_single = 0;
    hipStream_t cap = nullptr;
    int last_error = 0;
    ~SrPlan() {
        if (exec) hipGraphExecDestroy(exec);
        if (exec_chunk) hipGraphExecDestroy(exec_chunk);
        if (cap) hipStreamDestroy(cap);
        if (tiled_slab) (void)hipFree(tiled_slab);
        if (t2tbl) (void)hipFree(t2tbl);
        if (winu) (void)hipFree(winu);
        if (origin) (void)hipFree(origin);
        if (utt) (void)hipFree(utt);
    }

    int launch(const SkJob* jobs, int n, hipStream_t st, int force_tile = 0) {
        SkLaunch L;
        SR_TRY(sk_make_launch(L, jobs, n));
        L.force_tile = force_tile;
        return sk_launch(L, st);
    }

    // K segment A [B, K] . W[:, n0:] of a row-major [K, ldw] matrix, read from its fragment-major copy Wt where the plan
    // has one ((K >> 4) * 256 floats per 16-column tile)
    static SkSeg seg(const float* A, int K, const float* W, int ldw, const float* Wt, int n0 = 0) {
        const int blk = (K >> 4) * 256;
        return Wt ? sk_seg(A, K, Wt + (size_t)(n0 >> 4) * blk, blk, K, 2) : sk_seg(A, K, W + n0, ldw, K, 0);
    }

    // out [B, N] = act(A [B, K] . W [K, N] + bias)
    int linear(const float* A, int K, const float* W, const float* Wt, int N, const float* bias, float* out, int act,
               hipStream_t st) {
        SkJob j;
        sk_linear_job(j, seg(A, K, W, N, Wt), d.B, N, N, out, N);
        j.act = act;
        j.bias = bias;
        return launch(&j, 1, st);
    }

    // GRU step of a tier (ops.py:356-393): gates = sigm(h.Wg + x.U[:, :2D] + b[:2D]); cand = tanh((r*h).Wc + x.U[:, 2D:] +
    // b[2D:]); in-place h.  The Input linear rides in the step GEMMs as a second K segment: two launches, not three.
    // pre: x . U + bU arrives precomputed ([B, 3D]: gates | candidate) and only the recurrent product is left;
    // gates_done: the previous frame's sample kernel has left z and r*h already.
    // xs (skip stacks, layers above the first): U is [2D, 3D] and its rows D .. 2D-1 multiply the stack's input xs -- one
    // more K segment in both jobs, still two launches.
    int gru(const float* x, const float* U, const float* bU, const float* Wg, const float* Wc, float* h, hipStream_t st,
            const Tiled& t, const float* pre = nullptr, bool gates_done = false, const float* xs = nullptr) {
        const int D = d.D;
        const float* Us = xs ? U + (size_t)D * 3 * D : nullptr;
        SkJob j;
        if (!gates_done) {
            sk_gru_gates_job(j, d.B, D, h, d.z, d.r, d.rh);
            j.seg[j.nseg++] = seg(h, D, Wg, 2 * D, t.Wg);
            if (pre) { j.add = pre; j.ld_add = 3 * D; }
            else { j.seg[j.nseg++] = seg(x, D, U, 3 * D, t.U); j.bias = bU; }
            if (xs) j.seg[j.nseg++] = seg(xs, D, Us, 3 * D, nullptr);
            SR_TRY(launch(&j, 1, st));
        }
        sk_gru_cand_job(j, d.B, D, h, d.z, nullptr, h);
        j.seg[j.nseg++] = seg(d.rh, D, Wc, D, t.Wc);
        if (pre) { j.add = pre + 2 * D; j.ld_add = 3 * D; }
        else { j.seg[j.nseg++] = seg(x, D, U, 3 * D, t.U, 2 * D); j.bias = bU + 2 * D; }
        if (xs) j.seg[j.nseg++] = seg(xs, D, Us, 3 * D, nullptr, 2 * D);
        return launch(&j, 1, st);
    }

    // LSTM step of a tier layer (ops.py:505-553): pre = x . Win + b; gates = s . Wrec + pre (i | f | o | g);
    // c' = c*f + g*i; s' = tanh(c')*o.  s is the A operand of the step GEMM, so s' goes to a temporary first.
    // xs (skip stacks, layers above the first): Win is [2D, 4D], rows D .. 2D-1 multiply the stack's input xs.
    int lstm_layer(const float* x, const float* Win, const float* b, const float* Wrec, float* s, float* c, hipStream_t st,
                   const float* xs = nullptr) {
        const int D = d.D;
        if (!xs) {
            SR_TRY(linear(x, D, Win, nullptr, 4 * D, b, d.P, 0, st));
        } else {
            SkJob in;
            sk_linear_job(in, seg(x, D, Win, 4 * D, nullptr), d.B, 4 * D, 4 * D, d.P, 4 * D);
            in.seg[in.nseg++] = seg(xs, D, Win + (size_t)D * 4 * D, 4 * D, nullptr);
            in.bias = b;
            SR_TRY(launch(&in, 1, st));
        }
        SkJob j;
        sk_lstm_job(j, d.B, D, c, c, d.gate_ws, d.layer_tmp);
        j.seg[j.nseg++] = seg(s, D, Wrec, 4 * D, nullptr);
        j.add = d.P; j.ld_add = 4 * D;
        SR_TRY(launch(&j, 1, st));
        return (int)hipMemcpyAsync(s, d.layer_tmp, (size_t)d.B * D * sizeof(float), hipMemcpyDeviceToDevice, st);
    }

    // One step of a tier's RNN stack on input x [B,D]; returns the top layer's output (state) pointer.
    int stack_step(bool big, const float* x, const float** top, hipStream_t st) {
        if (d.n_rnn == 0) {  // single GRU layer, original fields
            if (big) SR_TRY(gru(x, d.big_U, d.big_bU, d.big_Wg, d.big_Wc, d.big_h, st, t_big));
            else SR_TRY(gru(x, d.frm_U, d.frm_bU, d.frm_Wg, d.frm_Wc, d.frm_h, st, t_frm));
            *top = big ? d.big_h : d.frm_h;
            return 0;
        }
        const float* const xs = x;  // the stack's input: what every layer above the first of a skip stack reads too
        for (int k = 0; k < d.n_rnn; ++k) {
            const float* const* Lk = big ? d.big_L[k] : d.frm_L[k];
            float* hs = big ? d.big_hs[k] : d.frm_hs[k];
            const float* in2 = has_skip && k > 0 ? xs : nullptr;
            if (d.lstm) SR_TRY(lstm_layer(x, Lk[0], Lk[1], Lk[2], hs, big ? d.big_cs[k] : d.frm_cs[k], st, in2));
            else SR_TRY(gru(x, Lk[0], Lk[1], Lk[2], Lk[3], hs, st, Tiled(), nullptr, false, in2));
            x = hs;
        }
        if (has_skip) {  // out = sum_k h_k . S_k + bS: one job, one K segment per layer (f32 sums inside the job)
            const float* const* S = big ? skip.big_S : skip.frm_S;
            float* out = big ? skip.big_sum : skip.frm_sum;
            SkJob j;
            sk_linear_job(j, d.B, d.D, d.D, out, d.D);
            for (int k = 0; k < d.n_rnn; ++k) j.seg[j.nseg++] = seg(big ? d.big_hs[k] : d.frm_hs[k], d.D, S[k], d.D, nullptr);
            j.bias = big ? skip.big_bS : skip.frm_bS;
            SR_TRY(launch(&j, 1, st));
            x = out;
        }
        *top = x;
        return 0;
    }

    // Packed runs: the streams that begin an utterance in this period (sr_start_kernel).  Everything a period reads that an
    // earlier period wrote is in this list: the sample history, the tiers' states, gpre and the sample kernel's carry; the
    // rest of the scratch (xf_big .. logits, pbig, pin, z, rh, P, gate_ws, layer_tmp) is written before it is read in
    // every period, and tbase belongs to the run, not to a stream.
    int start_rows(hipStream_t st) {
        SrStartArgs a{};
        a.starts = d.starts; a.tbase = d.tbase; a.samples = d.samples;
        a.B = d.B; a.D = d.D; a.T = d.T; a.BFS = d.BFS; a.len = d.BFS * d.T; a.q0 = d.Q / 2;
        const size_t D = d.D, row = (d.lstm ? 2 : 1) * D;
        auto add = [&](float* state, const float* h0) { a.state[a.nstate] = state; a.h0[a.nstate] = h0; ++a.nstate; };
        if (d.n_rnn == 0) {
            add(d.big_h, d.big_h0);
            add(d.frm_h, d.frm_h0);
        }
        for (int k = 0; k < d.n_rnn; ++k) {
            add(d.big_hs[k], d.big_h0 + k * row);
            add(d.frm_hs[k], d.frm_h0 + k * row);
            if (d.lstm) {  // h0 rows are [s | c]
                add(d.big_cs[k], d.big_h0 + k * row + D);
                add(d.frm_cs[k], d.frm_h0 + k * row + D);
            }
        }
        if (persist && winu) { a.gpre = gpre; a.gpre0 = gpre0; }
        if (persist) a.carry = srp_carry_keys(d.persist_ws, d.D, d.Q, groups);
        a.utt = utt; a.utt_seed = utt_seed; a.utt_temp = utt_temp; a.origin = origin;
        a.utt_top_k = utt_top_k; a.top_k = d.top_k;
        a.utt_top_p = utt_top_p; a.top_p = top_p;
        a.utt_min_p = utt_min_p; a.min_p = min_p;
        hipLaunchKernelGGL(sr_start_kernel, dim3(d.B), dim3(256), 0, st, a);
        return (int)hipGetLastError();
    }

    int period(hipStream_t st) {
        const int B = d.B, D = d.D, FS = d.FS, BFS = d.BFS, len = BFS * d.T;
        const float half_q = (float)(d.Q / 2);
        const int nfr = BFS / FS;
        if (d.starts) SR_TRY(start_rows(st));
        // ---- big-frame tier (three_tier.py:291-380), consumes samples[t-80:t] and features[t/80]
        {
            const int n = B * (BFS > d.feat_dim ? BFS : d.feat_dim);
            hipLaunchKernelGGL(sr_prep_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, d.samples, len, d.tbase, 0, BFS,
                               half_q, d.xf_big, B, d.features, d.feat_cur, d.feat_dim, BFS);
            SkJob in;  // gru_in = [xf_big | feat_cur] . [Win_frames ; Win_feats] + bin
            sk_linear_job(in, B, D, D, d.gru_in, D);
            in.seg[in.nseg++] = seg(d.xf_big, BFS, d.big_Win_frames, D, nullptr);
            in.seg[in.nseg++] = seg(d.feat_cur, d.feat_dim, d.big_Win_feats, D, nullptr);
            in.bias = d.big_bin;
            SR_TRY(launch(&in, 1, st));
            const float* top = nullptr;
            SR_TRY(stack_step(true, d.gru_in, &top, st));
            SR_TRY(linear(top, D, d.big_Wout, t_big.Wout, nfr * D, d.big_bout, d.big_out, 0, st));
            if (winu) {  // the big tier's share of every frame's pre-activations: pbig[(b, f)] = big_out[b, f*D : (f+1)*D] . U +
                         // (bin . U + bU), one step-kernel launch with one job per frame (the LDS-tiled GEMM would put the
                         // [B nfr, 3D] product on 48 workgroups of 128 x 128 x K: measured 75 us per period)
                // big_out [B, nfr D] is a [B nfr, D] matrix of (stream, frame) rows and pbig [B nfr, 3D] likewise: jobs of up
                // to 64 consecutive rows each (the step kernel's tallest tile), every job streaming U once -- 12 MB x
                // B nfr / 64 per period where one job per frame (32 rows) read it nfr times
                SkJob jobs[SK_MAXJOB];
                const int rows = B * nfr, RJ = 64;
                for (int r0 = 0; r0 < rows; r0 += RJ * SK_MAXJOB) {
                    int nj = 0;
                    for (int r = r0; r < rows && nj < SK_MAXJOB; r += RJ, ++nj) {
                        sk_linear_job(jobs[nj], seg(d.big_out + (size_t)r * D, D, d.frm_U, 3 * D, t_frm.U),
                                      rows - r < RJ ? rows - r : RJ, 3 * D, 3 * D, pbig + (size_t)r * 3 * D, 3 * D);
                        jobs[nj].bias = pbias;
                    }
                    SR_TRY(launch(jobs, nj, st));
                }
            }
        }
        for (int f = 0; f < nfr; ++f) {
            // ---- frame tier (three_tier.py:382-450), consumes samples[t-10:t] and big_out[:, (t/10)%8]
            const int toff = f * FS;
            // (on the persistent path the previous frame's sample kernel has already left this frame's input in gru_in)
            const float* ftop = nullptr;
            if (winu) {  // composed input: pin = xf . (Win . U) + pbig[f]  ([B, 3D]); the step GEMMs walk K = D
                // (persistent path: h . Wg of this frame's gates was made beside the previous frame's projection -- the last
                // frame of the previous period, or run()'s launch in front of the first one -- so the input kernel of a
                // period's first frame finishes the gates as the sample kernel does for the other frames)
                if (!persist)
                    hipLaunchKernelGGL(sr_frame_in_kernel, dim3(ceil_div(3 * D, 256), B), dim3(256), 0, st, d.samples, len,
                                       d.tbase, toff, FS, half_q, winu, (const float*)nullptr, pbig + (size_t)f * 3 * D,
                                       nfr * 3 * D, pin, 3 * D);
                else if (f == 0)
                    hipLaunchKernelGGL(sr_frame_in_kernel, dim3(ceil_div(3 * D, 256), B), dim3(256), 0, st, d.samples, len,
                                       d.tbase, toff, FS, half_q, winu, (const float*)nullptr, pbig + (size_t)f * 3 * D,
                                       nfr * 3 * D, pin, 3 * D, (const float*)gpre, (const float*)d.frm_h, d.z, d.rh, D);
                SR_TRY(gru(nullptr, d.frm_U, d.frm_bU, d.frm_Wg, d.frm_Wc, d.frm_h, st, t_frm, pin, persist));
                ftop = d.frm_h;
            } else {
                if (!persist || f == 0)
                    hipLaunchKernelGGL(sr_frame_in_kernel, dim3(ceil_div(D, 256), B), dim3(256), 0, st, d.samples, len, d.tbase,
                                       toff, FS, half_q, d.frm_Win, d.frm_bin, d.big_out + (size_t)f * D, nfr * D, d.gru_in, D);
                SR_TRY(stack_step(false, d.gru_in, &ftop, st));
            }
            if (persist && winu) {  // (last frame of the period: the gates' product of the next period's first frame)
                // the projection and, beside it, the recurrent product of the NEXT frame's gates (h' . Wg: it does not wait for
                // the frame's samples); the sample kernel finishes those gates at its end
                SkJob jobs[2];
                sk_linear_job(jobs[0], seg(ftop, D, Pout, FS * D, t_frm.Wout), B, FS * D, FS * D, d.frame_out, FS * D);
                jobs[0].bias = cb;
                sk_linear_job(jobs[1], seg(ftop, D, d.frm_Wg, 2 * D, t_frm.Wg), B, 2 * D, 2 * D, gpre, 2 * D);
                // (FS + 2) D columns = 768 column tiles at D = 1024: 16-column workgroups are three per CU; the heuristic's
                // 32-column ones (384) leave half the CUs with two streams and half with one (8.17 vs 8.07 us per sample)
                SR_TRY(launch(jobs, 2, st, 21));
            } else {
                SR_TRY(linear(ftop, D, persist ? Pout : d.frm_Wout, t_frm.Wout, FS * D, persist ? cb : d.frm_bout, d.frame_out, 0, st));
            }
            if (persist) {
                // ---- all FS sample steps of this frame in one launch: XCD-local persistent-thread kernel
                SrpArgs sa{};
                sa.tbase = d.tbase; sa.toff = toff; sa.samples = d.samples; sa.len = len;
                sa.B = B; sa.D = D; sa.Q = d.Q; sa.FS = FS; sa.nsteps = FS; sa.ngroups = groups;
                sa.t2tbl = t2tbl; sa.frame_out = d.frame_out; sa.ldf = FS * D;
                sa.W3 = d.W3; sa.b3 = d.b3; sa.W4 = d.W4; sa.b4 = d.b4;
                sa.logits = d.logits; sa.ws = d.persist_ws; sa.temperature = d.temperature; sa.seed = d.seed;
                sa.origin = origin; sa.utt = utt; sa.draw_mode = d.draw_mode; sa.top_k = srp_trunc_word(d.top_k, top_p, min_p, d.Q); sa.top_p = top_p;
                sa.min_p = min_p;
                sa.forced = forced; sa.logp = logp; sa.dlogp = dlogp; sa.kept = kept;
                if (f + 1 < nfr && winu) {  // the next frame of this period: its big-tier share is already known
                    sa.next_in = pin; sa.next_Win = winu; sa.next_bias = nullptr;
                    sa.next_add = pbig + (size_t)(f + 1) * 3 * D; sa.next_ld_add = nfr * 3 * D; sa.next_n = 3 * D;
                    sa.next_gpre = gpre; sa.next_h = d.frm_h; sa.next_z = d.z; sa.next_rh = d.rh;
                } else if (f + 1 < nfr) {
                    sa.next_in = d.gru_in; sa.next_Win = d.frm_Win; sa.next_bias = d.frm_bin;
                    sa.next_add = d.big_out + (size_t)(f + 1) * D; sa.next_ld_add = nfr * D;
                }
                {
                    static const int timing = env_int("PARROT_SR_TIMING", 0);
                    sa.pad = timing;
                }
                SR_TRY(srp_launch(sa, st));
                continue;
            }
            for (int i = 0; i < FS; ++i) {
                // ---- sample-level MLP (three_tier.py:452-515) + pick (ops.py:268-297)
                const int to = toff + i;
                hipLaunchKernelGGL(sr_embed_sum_kernel, dim3(ceil_div(D / 4, 256), B), dim3(256), 0, st, d.samples, len,
                                   d.tbase, to, FS, d.Q, D, d.emb_tbl, d.frame_out + (size_t)i * D, FS * D, d.o1);
                SR_TRY(linear(d.o1, D, d.W2, nullptr, D, d.b2, d.o2, SK_ACT_RELU, st));
                SR_TRY(linear(d.o2, D, d.W3, nullptr, D, d.b3, d.o3, SK_ACT_RELU, st));
                SR_TRY(linear(d.o3, D, d.W4, nullptr, d.Q, d.b4, d.logits, 0, st));
                hipLaunchKernelGGL(sr_pick_kernel, dim3(B), dim3(256), 0, st, d.logits, d.Q, d.samples, len, d.tbase, to,
                                   d.temperature, d.seed, (const unsigned long long*)origin, (const SrUttDraw*)utt, d.draw_mode,
                                   d.top_k, top_p, min_p, forced, logp, dlogp, kept);
            }
        }
        hipLaunchKernelGGL(sr_tick_kernel, dim3(1), dim3(64), 0, st, d.tbase, BFS, 0, (unsigned long long*)nullptr);
        return (int)hipGetLastError();
    }

    // The ring turns (sr_resume_kernel): everything else a period reads from the one before it -- the tiers' states, gpre,
    // and gpre0 of a packed plan -- stays where the last period left it.
    int resume_rows(hipStream_t st) {
        SrResumeArgs a{};
        a.tbase = d.tbase; a.samples = d.samples; a.origin = origin;
        a.B = d.B; a.T = d.T; a.BFS = d.BFS; a.len = d.BFS * d.T;
        if (persist) a.carry = srp_carry_keys(d.persist_ws, d.D, d.Q, groups);
        hipLaunchKernelGGL(sr_resume_kernel, dim3(1), dim3(256), 0, st, a);
        return (int)hipGetLastError();
    }

    int run(int periods, bool resume, hipStream_t st) {
        hipError_t e;
        if (resume) {
            SR_TRY(resume_rows(st));
        } else {
            // tbase starts at BFS (first 80 samples are Q_ZERO, set by the caller); `periods` periods follow (T-1: a whole run).
            hipLaunchKernelGGL(sr_tick_kernel, dim3(1), dim3(64), 0, st, d.tbase, d.BFS, 1, origin);
            e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
            if (utt) {  // every stream's first utterance: row 1 of the caller's arrays, prefix in slot 0
                hipLaunchKernelGGL(sr_utt_init_kernel, dim3(ceil_div(d.B, 256)), dim3(256), 0, st, utt, utt_seed + d.B,
                                   utt_temp + d.B, utt_top_k ? utt_top_k + d.B : (const int*)nullptr, d.top_k,
                                   utt_top_p ? utt_top_p + d.B : (const float*)nullptr, top_p,
                                   utt_min_p ? utt_min_p + d.B : (const float*)nullptr, min_p, d.B);
                e = hipGetLastError();
                if (e != hipSuccess) return (int)e;
            }
            if (persist && winu)  // h0 . Wg: the gates' recurrent product of the very first frame (see period())
                SR_TRY(linear(d.frm_h, d.D, d.frm_Wg, t_frm.Wg, 2 * d.D, nullptr, gpre, 0, st));
            if (persist && winu && d.starts)
                SR_TRY((int)hipMemcpyAsync(gpre0, gpre, (size_t)d.B * 2 * d.D * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        has_run = true;
        if (!d.use_graph) {
            for (int p = 0; p < periods; ++p) SR_TRY(period(st));
            return 0;
        }
        // Two graphs: one period, and SR_CHUNK periods back to back (a graph launch costs ~9 us of idle GPU between two
        // periods -- 0.1 us per sample; the chunk graph pays it once per SR_CHUNK periods).  tbase advances on the device.
        auto capture = [&](int n, hipGraphExec_t* out) -> int {
            if (!cap) {
                hipError_t ce = hipStreamCreateWithFlags(&cap, hipStreamNonBlocking);
                if (ce != hipSuccess) return (int)ce;
            }
            hipError_t ce = hipStreamBeginCapture(cap, hipStreamCaptureModeRelaxed);
            if (ce != hipSuccess) return (int)ce;
            int rc = 0;
            for (int q = 0; q < n && rc == 0; ++q) rc = period(cap);
            hipGraph_t graph = nullptr;
            ce = hipStreamEndCapture(cap, &graph);
            if (rc != 0) { if (graph) hipGraphDestroy(graph); return rc; }
            if (ce != hipSuccess) return (int)ce;
            ce = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
            hipGraphDestroy(graph);
            if (ce != hipSuccess) { *out = nullptr; return (int)ce; }
            return 0;
        };
        if (!exec) SR_TRY(capture(1, &exec));
        if (periods >= SR_CHUNK && !exec_chunk) SR_TRY(capture(SR_CHUNK, &exec_chunk));
        int left = periods;
        for (; exec_chunk && left >= SR_CHUNK; left -= SR_CHUNK) {
            e = hipGraphLaunch(exec_chunk, st);
            if (e != hipSuccess) return (int)e;
        }
        periods_left_single = left;
        for (int p = 0; p < periods_left_single; ++p) {
            e = hipGraphLaunch(exec, st);
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    }
};

}  // namespace

extern "C" {

int samplernn_generate_create(const SampleRnnGenDesc* desc, void** plan) { PH_ENTRY();
    if (!desc || !plan || desc->B < 1 || desc->T < 2 || desc->D < 4 || (desc->D & 3) || desc->FS < 1 ||
        desc->BFS % desc->FS != 0 || desc->Q < 2 || desc->n_rnn < 0 || desc->n_rnn > 5)
        return PARROT_ERR_BADARG;
    if (desc->starts && (!desc->big_h0 || !desc->frm_h0)) return PARROT_ERR_BADARG;
    // (draw_mode 1: every lane of the drawing wave owns Q / 64 codes)
    if (desc->draw_mode < 0 || desc->draw_mode > 1 || (desc->draw_mode == 1 && desc->Q % 64 != 0)) return PARROT_ERR_BADARG;
    // (top_k = 0 or >= Q: no truncation; the selection holds at most four codes per lane of one wave)
    if (desc->top_k < 0) return PARROT_ERR_BADARG;
    if (desc->top_k >= 1 && desc->top_k < desc->Q && desc->Q > 256) return PARROT_ERR_UNSUPPORTED;
    if (desc->n_rnn > 0) {
        if (desc->lstm && (!desc->gate_ws || !desc->layer_tmp)) return PARROT_ERR_BADARG;
        for (int k = 0; k < desc->n_rnn; ++k) {
            if (!desc->big_hs[k] || !desc->frm_hs[k] || (desc->lstm && (!desc->big_cs[k] || !desc->frm_cs[k])))
                return PARROT_ERR_BADARG;
            for (int q = 0; q < (desc->lstm ? 3 : 4); ++q)
                if (!desc->big_L[k][q] || !desc->frm_L[k][q]) return PARROT_ERR_BADARG;
        }
    }
    SrPlan* p = new (std::nothrow) SrPlan();
    if (!p) return PARROT_ERR_BADARG;
    p->d = *desc;
    const int max_groups = srp_max_groups(), groups = srp_groups_for(desc->B, max_groups);
    p->persist = desc->persist_ws && srp_eligible(desc->B, desc->D, desc->Q, desc->FS, max_groups) &&
                 desc->persist_ws_floats >= srp_ws_floats(desc->D, desc->Q, groups) && srp_prepare(desc->D) == 0 &&
                 srp_init_ws(desc->persist_ws, desc->D, desc->Q, groups) == 0 && p->make_composed() == 0;
    p->groups = p->persist ? groups : 0;
    p->make_tiled();  // (after the decision: the persistent path tiles the composed projection)
    p->make_winu();
    if (p->make_origin() != 0) { delete p; return PARROT_ERR_BADARG; }
    *plan = p;
    return 0;
}

long long samplernn_persist_floats(const SampleRnnGenDesc* desc) { PH_ENTRY();
    const int max_groups = srp_max_groups();
    if (!desc || !srp_eligible(desc->B, desc->D, desc->Q, desc->FS, max_groups)) return 0;
    return srp_ws_floats(desc->D, desc->Q, srp_groups_for(desc->B, max_groups));
}

int samplernn_generate_is_persistent(void* plan) { PH_ENTRY();
    return plan && static_cast<SrPlan*>(plan)->persist ? 1 : 0;
}

int samplernn_generate_persist_groups(void* plan) { PH_ENTRY();
    return plan ? static_cast<SrPlan*>(plan)->groups : 0;
}

// (no HIP call, not even PH_ENTRY's: the group arithmetic is testable on a machine without a device)
int samplernn_persist_groups_dry(int B, int max_groups) { return srp_groups_for(B, max_groups); }

int samplernn_generate_status(void* plan) { PH_ENTRY();
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p) return PARROT_ERR_BADARG;
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return (int)e;
    if (p->last_error) return p->last_error;
    return p->persist ? srp_status(p->d.persist_ws) : 0;
}

int samplernn_generate_run_segment(void* plan, int n_periods, int resume, void* stream) { PH_ENTRY();
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || n_periods < 1 || n_periods > p->d.T - 1 || (resume && !p->has_run)) return PARROT_ERR_BADARG;
    const int rc = p->run(n_periods, resume != 0, (hipStream_t)stream);
    if (rc != 0 && p->last_error == 0) p->last_error = rc;
    return rc;
}

// (the argument checks in front of any HIP call, PH_ENTRY's included: they are testable on a machine without a device)
int samplernn_generate_set_utterance_draws(void* plan, const unsigned long long* utt_seed, const float* utt_temp) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !utt_seed || !utt_temp) return PARROT_ERR_BADARG;
    if (p->has_run) return PARROT_ERR_BADARG;  // the period graphs hold the pointers by value
    PH_ENTRY();
    return p->set_utt(utt_seed, utt_temp);
}

// (no HIP call at all: the pointer is handed to the kernels that fill the entries)
int samplernn_generate_set_utterance_top_k(void* plan, const int* utt_top_k) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !utt_top_k || !p->utt) return PARROT_ERR_BADARG;  // only after samplernn_generate_set_utterance_draws
    if (p->has_run) return PARROT_ERR_BADARG;                    // the period graphs hold the pointers by value
    if (p->d.Q > 256) return PARROT_ERR_UNSUPPORTED;
    p->utt_top_k = utt_top_k;
    return 0;
}

// The plan's nucleus.  (No HIP call: the value is handed to the kernels by the launches of the first run.)
int samplernn_generate_set_top_p(void* plan, float top_p) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !(top_p >= 0.f)) return PARROT_ERR_BADARG;  // (a NaN compares false)
    if (p->has_run) return PARROT_ERR_BADARG;             // the period graphs hold the arguments by value
    if (top_p > 0.f && top_p < 1.f && p->d.Q > 256) return PARROT_ERR_UNSUPPORTED;
    p->top_p = top_p;
    return 0;
}

// (no HIP call either: the pointer is handed to the kernels that fill the entries)
int samplernn_generate_set_utterance_top_p(void* plan, const float* utt_top_p) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !utt_top_p || !p->utt) return PARROT_ERR_BADARG;  // only after samplernn_generate_set_utterance_draws
    if (p->has_run) return PARROT_ERR_BADARG;
    if (p->d.Q > 256) return PARROT_ERR_UNSUPPORTED;
    p->utt_top_p = utt_top_p;
    return 0;
}

// Forced samples and per-sample log-probabilities.  (No HIP call: the pointers are handed to the sample kernels of both
// paths by the launches of the first run.)
int samplernn_generate_set_forced(void* plan, const int* forced) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !forced) return PARROT_ERR_BADARG;
    if (p->has_run) return PARROT_ERR_BADARG;  // the period graphs hold the pointers by value
    p->forced = forced;
    return 0;
}

int samplernn_generate_set_log_probs(void* plan, float* logp) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !logp) return PARROT_ERR_BADARG;
    if (p->has_run) return PARROT_ERR_BADARG;
    p->logp = logp;
    return 0;
}

// What each draw kept.  (No HIP call, like the two above.)
int samplernn_generate_set_draw_stats(void* plan, float* draw_logp, int* kept) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !draw_logp || !kept) return PARROT_ERR_BADARG;
    if (p->has_run) return PARROT_ERR_BADARG;
    p->dlogp = draw_logp;
    p->kept = kept;
    return 0;
}

// Skip-connection stacks.  (No HIP call: the pointers are handed to the step jobs by the launches of the first run.)
int samplernn_generate_set_skip_stacks(void* plan, const SampleRnnSkipStacks* skip) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !skip) return PARROT_ERR_BADARG;
    if (p->d.n_rnn < 2) return PARROT_ERR_UNSUPPORTED;  // (the single-GRU plan has n_rnn = 0; no one-layer skip stack exists)
    if (p->has_run) return PARROT_ERR_BADARG;           // the period graphs hold the pointers by value
    if (!skip->big_bS || !skip->frm_bS || !skip->big_sum || !skip->frm_sum) return PARROT_ERR_BADARG;
    for (int k = 0; k < p->d.n_rnn; ++k)
        if (!skip->big_S[k] || !skip->frm_S[k]) return PARROT_ERR_BADARG;
    p->skip = *skip;
    p->has_skip = true;
    return 0;
}

// The plan's min_p.  (No HIP call, like the nucleus.)
int samplernn_generate_set_min_p(void* plan, float min_p) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !(min_p >= 0.f && min_p <= 1.f)) return PARROT_ERR_BADARG;  // (a NaN compares false)
    if (p->has_run) return PARROT_ERR_BADARG;                             // the period graphs hold the arguments by value
    if (min_p > 0.f && p->d.Q > 256) return PARROT_ERR_UNSUPPORTED;
    p->min_p = min_p;
    return 0;
}

// (no HIP call either: the pointer is handed to the kernels that fill the entries)
int samplernn_generate_set_utterance_min_p(void* plan, const float* utt_min_p) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !utt_min_p || !p->utt) return PARROT_ERR_BADARG;  // only after samplernn_generate_set_utterance_draws
    if (p->has_run) return PARROT_ERR_BADARG;
    if (p->d.Q > 256) return PARROT_ERR_UNSUPPORTED;
    p->utt_min_p = utt_min_p;
    return 0;
}

// Conditioning frames from device memory into rows first .. first + rows - 1 of the plan's features (sr_stage.hip).  (The
// argument checks in front of any HIP call: they are testable on a machine without a device.)  The descriptor declares
// `features` const because the generation kernels only read it; the buffer is the caller's and writable.
int samplernn_generate_stage_features(void* plan, const float* src, long long src_rows, int src_ld, const int* index, int first,
                                      int rows, void* stream) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    if (!p || !src || !index || first < 0 || rows < 1 || (long long)first + rows > p->d.T) return PARROT_ERR_BADARG;
    if (src_ld < p->d.feat_dim || src_rows < 1) return PARROT_ERR_BADARG;
    PH_ENTRY();
    return sr_stage_features(const_cast<float*>(p->d.features), p->d.B, p->d.feat_dim, src, src_rows, src_ld, index, first, rows,
                             (hipStream_t)stream);
}

int samplernn_generate_run(void* plan, void* stream) {
    SrPlan* p = static_cast<SrPlan*>(plan);
    return samplernn_generate_run_segment(plan, p ? p->d.T - 1 : 0, 0, stream);
}

int samplernn_generate_destroy(void* plan) { PH_ENTRY();
    delete static_cast<SrPlan*>(plan);
    return 0;
}

}  // extern "C"

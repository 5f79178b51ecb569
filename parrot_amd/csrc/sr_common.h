// Device helpers of the SampleRNN persistent-thread sample kernel (sr_persist.hip): XCD teams, EMPTY-slot hand-offs that
// stay in the XCD's L2, the register-resident [4 streams x CU columns] product, DPP wave reductions.
#pragma once
#include "common.h"

namespace {

constexpr int SRP_THREADS = 512, SRP_TEAM = 32, SRP_NTEAMS = 8, SRP_ROWS = 4, SRP_Q = 256;
constexpr int SRP_SYNC_WORDS = 1024;  // [256 + 32 team] arrivals per team (counted, not waited for), [512] abort, [513] fault code,
                                      // [600 ..) phase stamps of a timed launch (PARROT_SR_TIMING)
constexpr int SRP_MAXHIST = 64;       // FS + nsteps
constexpr int SRP_GMAX = 12;          // table rows of the gather requested in one batch (FS - 1 <= SRP_GMAX; else a loop)
constexpr int SRP_MAXGROUPS = 8;      // row groups of SRP_ROWS * SRP_NTEAMS streams one launch may take (PARROT_SR_PERSIST_GROUPS)
// f32x4 hand-off slots per (row group, team) in the workspace: x1, x2 [D] and the logits [Q]
__host__ __device__ constexpr int srp_team_vecs(int D, int Q) { return 2 * D + Q; }
// Carry between consecutive launches, per (row group, team), behind the hand-off slots of all groups: [0] the sample index
// it is for (-1: none), [16 ..) the team's last FS samples [4][SRP_CARRY_HIST], then per CU the table part of the next first
// gather [32][4][DC <= 32].  Blocks of both kinds are numbered group * SRP_NTEAMS + team.
constexpr int SRP_CARRY_HIST = 32;
constexpr int SRP_CARRY_WORDS = 16 + SRP_ROWS * SRP_CARRY_HIST + SRP_TEAM * SRP_ROWS * 32;
__host__ __device__ constexpr long long srp_carry_base(int D, int Q, int groups) {
    return SRP_SYNC_WORDS + (long long)groups * SRP_NTEAMS * srp_team_vecs(D, Q) * 4;
}

__device__ __forceinline__ int srp_xcc() {
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return (int)(v & 7);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t srp_rsrc(const void* p) {
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    void* q = (void*)(((unsigned long long)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(q, 0, 0x7fffffff, 0x00020000);
}
// sc1 load: misses in the CU's vector cache, served by the XCD's L2 (where the team's stores have landed)
__device__ __forceinline__ f32x4 srp_ld(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 16));
}

// Hand-off slots are 16 bytes = one value for each of the team's 4 streams.  An empty slot holds a NaN with a payload
// arithmetic never produces; a 16-byte store replaces it atomically in the L2, so a consumer simply re-reads a slot
// until it is full: no store acknowledgement, arrival counter or flag poll sits between producer and consumer.
constexpr unsigned SRP_EMPTY = 0x7FC0DEADu;
__device__ __forceinline__ f32x4 srp_empty() {
    const float e = __uint_as_float(SRP_EMPTY);
    return (f32x4){e, e, e, e};
}
__device__ __forceinline__ bool srp_is_empty(const f32x4& v) {
    return __float_as_uint(v[0]) == SRP_EMPTY || __float_as_uint(v[3]) == SRP_EMPTY;
}

// 100 MHz wall clock (timing aid, PARROT_SR_TIMING=1: workgroup 0 of team 0 stamps the phase boundaries of every step
// into sync words 600..)
__device__ __forceinline__ unsigned long long srp_clock() {
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

struct SrpShared {
    int ok;
    int hist[SRP_ROWS][SRP_MAXHIST];
    float mx[SRP_ROWS];
    // per-utterance draw entries of the group's rows (SrpArgs::utt; unused without): parked here, not in registers
    float utemp[SRP_ROWS];
    int utopk[SRP_ROWS];
    float utopp[SRP_ROWS];
    int ulast[SRP_ROWS];  // the highest kept code of a truncated sequential draw (srp_kernel's pick)
    int upad;
    unsigned long long useed[SRP_ROWS], uoff[SRP_ROWS];
    // forced codes of the launch's steps for the group's rows (SrpArgs::forced; unused without), -1 = the step picks freely.
    // Behind everything else: the offsets of the fields above are the ones they had.
    int forced[SRP_ROWS][SRP_MAXHIST];
    // the rows' min_p (samplernn_generate_set_min_p: the entries', or the plan's without entries), written by every prologue
    float uminp[SRP_ROWS];
    // the kept set of a truncated sequential draw as the ballots of the lanes' kept bits (word m, bit l: code l + 64 m), parked
    // for the statistics behind the pick (SrpArgs::dlogp; srp_fx_kernel only)
    unsigned long long ukeepm[SRP_ROWS][SRP_Q / 64];
    // SrpArgs::dlogp / kept as the prologue parks them: read from here inside the step loop, not from the arguments
    float* dlogp;
    int* kept;
};
static_assert(sizeof(SrpShared) % 8 == 0, "SrpShared holds 64-bit words");

// Load a hand-off slot, re-reading until it is full (bounded: ~1 s, then the abort word is raised).
__device__ __forceinline__ f32x4 srp_take(__amdgpu_buffer_rsrc_t r, unsigned byte_off, unsigned* abort_, SrpShared* sh) {
    f32x4 v = srp_ld(r, byte_off);
    unsigned n = 0;
    while (srp_is_empty(v)) {
        if ((++n & 1023u) == 0u) {
            if (__hip_atomic_load(abort_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { sh->ok = 0; break; }
            if (n > (1u << 21)) {
                __hip_atomic_store(abort_, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(abort_ + 1, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                sh->ok = 0;
                break;
            }
        }
        __builtin_amdgcn_s_sleep(1);
        v = srp_ld(r, byte_off);
    }
    return v;
}

// f32x4 += the same vector of the lane selected by a DPP control (all four components)
template <int CTRL>
__device__ __forceinline__ f32x4 srp_dpp_add(const f32x4& v) {
    f32x4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        r[c] = v[c] + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[c]), CTRL, 0xf, 0xf, true));
    return r;
}

// out[4 rows][CC columns of this CU] = sum_k a[k][row] * W[k][col].  Thread (sl = tid & 7, g = (tid >> 3) % GG,
// sh = tid / (8 GG)) owns K-slice s = 8 sh + sl, i.e. k = kk * SS + s, and columns 4g .. 4g+3 of the CU's slice; its
// weights w(kk) are W[k][4g .. 4g+3] (VGPRs).  The 8 slices of neighbouring lanes
// are added with DPP (quad swaps, then half-row mirror: a fixed tree), the 64 / GG lane groups through LDS in group
// order.  Result: threads tid < CC return the finished f32x4 (4 rows) of CU column 4 * (tid % GG) + tid / GG.
// Wave-wide max / min with every lane receiving the result: quad swaps, half-row and row mirrors on the DPP path (no LDS
// crossbar as __shfl_xor would use: ~100 clocks instead of ~1200 for the six levels), the four row results through
// v_readlane.
template <int CTRL>
__device__ __forceinline__ float srp_dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int srp_dpp_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }
__device__ __forceinline__ float srp_wave_max(float v) {
    v = fmaxf(v, srp_dpp_f<0xB1>(v));
    v = fmaxf(v, srp_dpp_f<0x4E>(v));
    v = fmaxf(v, srp_dpp_f<0x141>(v));
    v = fmaxf(v, srp_dpp_f<0x140>(v));
    const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(a, b), fmaxf(c, d));
}
__device__ __forceinline__ int srp_wave_min(int v) {
    v = min(v, srp_dpp_i<0xB1>(v));
    v = min(v, srp_dpp_i<0x4E>(v));
    v = min(v, srp_dpp_i<0x141>(v));
    v = min(v, srp_dpp_i<0x140>(v));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// argmax of row r of the team's logits lg[Q] (4 streams per vector), lowest index on ties (numpy / Theano argmax):
// every lane returns the index and, through best, the maximum.
template <int Q>
__device__ __forceinline__ int srp_argmax_row(const f32x4* __restrict__ lg, int r, int lane, float& best) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int m = 0; m < Q / 64; ++m) {
        const float v = lg[lane + 64 * m][r];
        if (v > bv) { bv = v; bi = lane + 64 * m; }
    }
    best = srp_wave_max(bv);
    return srp_wave_min(bv == best ? bi : 0x7fffffff);
}

// Top-k truncation of a draw (SampleRnnGenDesc::top_k): the kept set is the k codes that come first when the codes are
// ordered by logit descending, then by code index ascending (a tie at the cut-off goes to the lower index, the argmax's rule).
// srp_order_image: the order-preserving unsigned image of a float32 logit, a > b <=> image(a) > image(b); -0.0 and +0.0, equal
// as logits, share one image.  Image 0 belongs to a NaN pattern no logit holds: it marks "no code" (a lane's padding).
__device__ __forceinline__ unsigned srp_order_image(float v) {
    unsigned u = __float_as_uint(v);
    u = u == 0x80000000u ? 0u : u;
    return u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
}
// Selection by one whole wave, whatever codes a lane holds: f[j] = the image of the lane's j-th logit (0: no code),
// idx[j] = its code index in 0 .. 255, 1 <= k < the number of codes, k wave-uniform.  Returns the lane's kept codes, bit j.
// A binary search over the 40-bit key (image, 255 - index), most significant bit first.  32 rounds find V = the largest
// image that at least k codes reach.  Then every code gets its rank in the cut-off's tie, t = 511 above V, 256 - index at V,
// 0 below, and 8 rounds find Y = the largest bound in 0 .. 255 that at least k codes exceed: the kept codes are those with
// t > Y -- all above V and the lowest indices of the tie.  A round is N compares, N ballots and their popcounts; the state
// (V, Y) is scalar and no lane mask outlives its round; the control flow is uniform; no LDS.
template <int N>
__device__ __forceinline__ unsigned srp_topk_keep(const unsigned (&f)[N], const int (&idx)[N], int k) {
    unsigned v = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned x = v | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) cnt += (int)__popcll(__ballot(f[j] >= x));
        v = cnt >= k ? x : v;
    }
    unsigned t[N];
#pragma unroll
    for (int j = 0; j < N; ++j) t[j] = f[j] > v ? 511u : f[j] == v ? (unsigned)(256 - idx[j]) : 0u;
    unsigned y = 0;
#pragma unroll 1
    for (int bit = 7; bit >= 0; --bit) {
        const unsigned x = y | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) cnt += (int)__popcll(__ballot(t[j] > x));
        y = cnt >= k ? x : y;
    }
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) keep |= t[j] > y ? 1u << j : 0u;
    return keep;
}
// The highest kept code of the wave (every lane receives it): what a sequential walk falls through to
template <int N>
__device__ __forceinline__ int srp_topk_last(unsigned keep, const int (&idx)[N]) {
    int hi = -1;
#pragma unroll
    for (int j = 0; j < N; ++j) hi = (keep >> j) & 1u ? max(hi, idx[j]) : hi;
    return -srp_wave_min(-hi);
}

// Top-p (nucleus) truncation of a draw (samplernn_generate_set_top_p): among the codes K that top-k left (all of them without),
// ordered as above, the kept set is the shortest prefix whose mass reaches p times the mass of K.  srp_wave_sum: the mass of
// one term per lane as a fixed tree of round-to-nearest float32 adds, every lane receiving the same bits -- quad swaps, half-row
// and row mirrors on the DPP path (both operands of each add hold the same two sub-sums, so the lanes of a row agree), then
// rows 0+1 and 2+3 and the two halves with the gfx950 row / half-wave swaps: ((r0 + r1) + (r2 + r3)).
__device__ __forceinline__ float srp_wave_sum(float v) {
    // (every lane has a source under these four controls, so "0 where there is none" never applies: written that way, the
    // DPP operand folds into the add -- one instruction per level instead of a copy, the DPP move and the add)
    v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true)));   // quad_perm [1,0,3,2]
    v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, true)));   // quad_perm [2,3,0,1]
    v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, true)));  // row_half_mirror
    v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, true)));  // row_mirror
    const unsigned u = __float_as_uint(v);
    const auto q = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const unsigned h = __float_as_uint(__fadd_rn(__uint_as_float(q[0]), __uint_as_float(q[1])));
    const auto w = __builtin_amdgcn_permlane32_swap(h, h, false, false);
    return __fadd_rn(__uint_as_float(w[0]), __uint_as_float(w[1]));
}
// (the sum as a scalar's bit pattern: sums of terms >= 0 compare as their patterns do as integers)
__device__ __forceinline__ int srp_wave_mass(float v) { return __builtin_amdgcn_readfirstlane(__float_as_int(srp_wave_sum(v))); }
// Selection by one whole wave, the sibling of srp_topk_keep and as indifferent to which codes a lane holds: f and idx as
// there, e[j] = the term of the lane's j-th code with 0.0f already in place of every code outside K (and of "no code"),
// 0 < p < 1 wave-uniform.  Returns the lane's kept codes, bit j.
// The mass of a set S of codes is M(S) = srp_wave_sum(((e'_0 + e'_1) + ...) + e'_{N-1}), e'_j = e[j] for a code of S and 0.0f
// for any other: the lane's codes left to right, then the tree above -- one fixed tree of round-to-nearest adds of terms
// >= 0 for every S, so S within S' gives M(S) <= M(S'), and the search below is over a monotone predicate.  The bar is
// need = p * M(K), one float32 product (> 0: the argmax code is in K and its term is 1).  32 rounds find V = the largest
// image with M({image >= V}) >= need, then 8 rounds over srp_topk_keep's tie rank t find Y = the largest bound in 0 .. 255
// with M({t > Y}) >= need; the kept codes are those with t > Y: every code above V and the lowest indices at V, the shortest
// prefix of the order that reaches the bar, never empty.  Masses and the bar are non-negative floats, which compare as
// their bit patterns do as integers: V, Y, the mass of a round and the bar are scalars, the control flow is uniform, no LDS.
template <int N>
__device__ __forceinline__ unsigned srp_topp_keep(const unsigned (&f)[N], const int (&idx)[N], const float (&e)[N], float p) {
    float s = e[0];
#pragma unroll
    for (int j = 1; j < N; ++j) s = __fadd_rn(s, e[j]);
    const int need = __float_as_int(p * __int_as_float(srp_wave_mass(s)));
    unsigned v = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned x = v | (1u << bit);
        s = f[0] >= x ? e[0] : 0.f;
#pragma unroll
        for (int j = 1; j < N; ++j) s = __fadd_rn(s, f[j] >= x ? e[j] : 0.f);
        v = srp_wave_mass(s) >= need ? x : v;
    }
    unsigned t[N];
#pragma unroll
    for (int j = 0; j < N; ++j) t[j] = f[j] > v ? 511u : f[j] == v ? (unsigned)(256 - idx[j]) : 0u;
    unsigned y = 0;
#pragma unroll 1
    for (int bit = 7; bit >= 0; --bit) {
        const unsigned x = y | (1u << bit);
        s = t[0] > x ? e[0] : 0.f;
#pragma unroll
        for (int j = 1; j < N; ++j) s = __fadd_rn(s, t[j] > x ? e[j] : 0.f);
        y = srp_wave_mass(s) >= need ? x : y;
    }
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) keep |= t[j] > y ? 1u << j : 0u;
    return keep;
}

// Min-p truncation of a draw (samplernn_generate_set_min_p): a code is kept iff its term e = expf((lg - max) / T), as the draw
// computes it, is >= min_p -- the argmax's term is exactly 1.0f, so with 0 < min_p <= 1 the set is never empty.  e[j] = the
// term of the lane's j-th code, 0.0f already in place of a code the truncations in front dropped (and of "no code"): 0 < min_p
// fails those, so the result is the intersection.  min_p wave-uniform.  Returns the lane's kept codes, bit j.  N compares:
// no rounds, no LDS, no cross-lane traffic.
template <int N>
__device__ __forceinline__ unsigned srp_minp_keep(const float (&e)[N], float min_p) {
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) keep |= e[j] >= min_p ? 1u << j : 0u;
    return keep;
}

// 24-bit uniform of a seeded draw: splitmix64 finaliser of key ^ K1 * counter, the middle of one of 2^24 cells of (0, 1)
__device__ __forceinline__ float srp_u01(unsigned long long key, unsigned long long ctr) {
    unsigned long long x = key ^ (0x9E3779B97F4A7C15ull * ctr);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return (float)((x >> 40) + 0.5) * (1.0f / 16777216.0f);
}

// Wave-parallel seeded draw (SampleRnnGenDesc::draw_mode = 1) by one whole wave: inverse-CDF pick among Q = 64 n codes
// whose terms e_q >= 0 lane `lane` delivers for its n contiguous codes, term(j) = e_{n lane + j} (called twice with the
// same bits).  The CDF is a fixed tree of plain float32 adds (__fadd_rn: never contracted, never reassociated):
//   p_l = ((e_{nl} + e_{nl+1}) + ...)                      the lane's partial, left to right
//   w_l = inclusive Hillis-Steele scan of p inside each row of 16 lanes, offsets 1, 2, 4, 8 (DPP row_shr with bound_ctrl:
//         a lane without a source adds the 0 it is handed, exact for terms >= 0)
//   s_l = w_l (row 0), R_{k-1} + w_l (row k) with the row totals chained R_0 = T_0, R_1 = R_0 + T_1, R_2 = R_1 + T_2
// tot = s_63, u = u01 * tot, l* = the lowest lane with u < s_l (none: the pick is Q - 1), and inside l* the terms are added
// one at a time to s_{l*-1} (0 for lane 0): the first code with u < c, or the lane's last code.  Every lane returns the pick.
// TK (a truncated draw: the terms of the codes outside the kept set are 0.0f, lk = the lane's highest kept code, -1 for
// none): both fall-through picks become the highest kept code not above the one they name without truncation -- the
// highest kept code of all for Q - 1, the highest kept code of lanes 0 .. l* for the lane's last code (there is one: u < s_l*
// needs s_l* > 0, and a sum of masked terms alone is exactly 0).  TK = false: the code as it was.
template <bool TK = false, class F>
__device__ __forceinline__ int srp_scan_draw(F term, int n, int lane, float u01, int lk = -1) {
    float p = term(0);
    for (int j = 1; j < n; ++j) p = __fadd_rn(p, term(j));
    float w = p;
    w = __fadd_rn(w, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(w), 0x111, 0xf, 0xf, true)));  // row_shr:1
    w = __fadd_rn(w, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(w), 0x112, 0xf, 0xf, true)));  // row_shr:2
    w = __fadd_rn(w, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(w), 0x114, 0xf, 0xf, true)));  // row_shr:4
    w = __fadd_rn(w, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(w), 0x118, 0xf, 0xf, true)));  // row_shr:8
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), 15));
    const float r1 = __fadd_rn(r0, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), 31)));
    const float r2 = __fadd_rn(r1, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), 47)));
    // (the row number is made opaque here: as a loop invariant of the caller its three compare masks would be kept in
    // six scalar registers across the persistent kernel's whole step loop, which has none to spare)
    int row = lane >> 4;
    asm volatile("" : "+v"(row));
    const float s =row == 0 ? w : __fadd_rn(row == 1 ? r0 : row == 2 ? r1 : r2, w);
    const float u = u01 * __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), 63));
    const unsigned long long hit = __ballot(u < s);
    const unsigned long long has = TK ? __ballot(lk >= 0) : 0ull;  // lanes that hold a kept code
    // the highest kept code of lanes 0 .. l (no such lane, which cannot happen: the lowest kept code)
    auto kept_up_to = [&](int l) {
        const unsigned long long m = has & (~0ull >> (63 - l));
        const int src = m ? 63 - (int)__builtin_clzll(m) : (int)__builtin_ctzll(has | (1ull << 63));
        return __builtin_amdgcn_readlane(lk, __builtin_amdgcn_readfirstlane(src));
    };
    if (hit == 0) return TK ? kept_up_to(63) : 64 * n - 1;
    const int ls = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(hit));
    const float below = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), max(ls - 1, 0)));
    int pick = TK ? kept_up_to(ls) : n * ls + n - 1;
    if (lane == ls) {
        float c = ls == 0 ? 0.f : below;
        for (int j = 0; j < n; ++j) {
            c = __fadd_rn(c, term(j));
            if (u < c) { pick = n * ls + j; break; }
        }
    }
    return __builtin_amdgcn_readlane(pick, ls);
}

// v + the same vector of the lane 16 (ROWS = 16: neighbouring row) or 32 (other half of the wave) lanes away
template <int ROWS>
__device__ __forceinline__ f32x4 srp_swap_add(const f32x4& v) {
    f32x4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned u = __float_as_uint(v[c]);
        if (ROWS == 16) {
            const auto q = __builtin_amdgcn_permlane16_swap(u, u, false, false);
            r[c] = __uint_as_float(q[0]) + __uint_as_float(q[1]);
        } else {
            const auto q = __builtin_amdgcn_permlane32_swap(u, u, false, false);
            r[c] = __uint_as_float(q[0]) + __uint_as_float(q[1]);
        }
    }
    return r;
}

// Fold of a product's per-thread partial sums acc[r] (stream r, the thread's 4 columns): the 8 K-slices of neighbouring
// lanes with DPP (quad swaps, then half-row mirror: a fixed tree), the 64 / GG lane groups through LDS in group order.
// Threads tid < 4 GG return the finished f32x4 (4 streams) of CU column 4 * (tid % GG) + tid / GG.
template <int GG>
__device__ __forceinline__ void srp_reduce(f32x4 (&acc)[4], f32x4* __restrict__ red, f32x4& out, int tid,
                                           unsigned long long* tp = nullptr) {
    constexpr int CC = 4 * GG, GROUPS = 64 / GG;
    const int sl = tid & 7, g = (tid >> 3) % GG, shi = tid / (8 * GG);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        acc[r] = srp_dpp_add<0xB1>(acc[r]);   // quad_perm [1,0,3,2]
        acc[r] = srp_dpp_add<0x4E>(acc[r]);   // quad_perm [2,3,0,1]
        acc[r] = srp_dpp_add<0x141>(acc[r]);  // row_half_mirror
    }
    if (tp) tp[1] = srp_clock();
    if (sl == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) red[shi * CC + j * GG + g] = (f32x4){acc[0][j], acc[1][j], acc[2][j], acc[3][j]};
    }
    __syncthreads();
    if (tp) tp[2] = srp_clock();
    // The GROUPS partial sums of each of the CC column vectors: wave 0 takes four of them per lane in ONE batch of LDS
    // reads (lane = part * CC + column) and adds the 64 / CC parts across lanes on the VALU -- row rotate, then the
    // gfx950 row / half-wave swaps.  (Round 5 had threads tid < CC walk the GROUPS partials four at a time: eight
    // dependent LDS round trips for the output layer, 1.1 us of the step.)
    if (tid < 64) {
        static_assert(GROUPS * CC == 256, "64 lanes x 4 partials");
        const int c = tid % CC, part = tid / CC;
        const f32x4 p0 = red[(4 * part + 0) * CC + c], p1 = red[(4 * part + 1) * CC + c];
        const f32x4 p2 = red[(4 * part + 2) * CC + c], p3 = red[(4 * part + 3) * CC + c];
        f32x4 v = (p0 + p1) + (p2 + p3);
        if (CC <= 8) v = srp_dpp_add<0x128>(v);  // row_ror:8
        if (CC <= 16) v = srp_swap_add<16>(v);
        out = srp_swap_add<32>(v);
    }
    if (tp) tp[3] = srp_clock();
}

template <int KPP, int GG>
__device__ __forceinline__ void srp_layer(const f32x4* __restrict__ act, const f32x4 (&w)[KPP], f32x4* __restrict__ red,
                                          f32x4& out, int tid, unsigned long long* tp = nullptr) {
    constexpr int SS = SRP_THREADS / GG;
    const int s = 8 * (tid / (8 * GG)) + (tid & 7);
    f32x4 acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // Activation reads run PF iterations ahead of the FMAs that use them, pinned by scheduling barriers: left alone the
    // scheduler (register pressure near the limit) emits read, wait, 8 FMAs, read, wait ... -- an LDS latency per step of K.
    constexpr int PF = KPP < 4 ? KPP : 4;
    f32x4 buf[PF];
#pragma unroll
    for (int j = 0; j < PF; ++j) buf[j] = act[j * SS + s];
#pragma unroll
    for (int kk = 0; kk < KPP; ++kk) {
        __builtin_amdgcn_sched_barrier(0);
        const f32x4 a = buf[kk % PF];
        const f32x4 wv = w[kk];
        // acc[r] = the 4 columns of stream r.  The scalar operand is the (transient) activation: broadcasting the
        // loop-invariant weights instead makes the compiler keep a 4-register splat of every weight alive.
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += a[r] * wv;
        if (kk + PF < KPP) {
            __builtin_amdgcn_sched_barrier(0);
            buf[kk % PF] = act[(kk + PF) * SS + s];
        }
    }
    if (tp) tp[0] = srp_clock();
    srp_reduce<GG>(acc, red, out, tid, tp);
}

}  // namespace

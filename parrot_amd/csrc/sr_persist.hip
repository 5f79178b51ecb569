// SampleRNN sample-level MLP as a persistent-thread kernel (gfx950).
//
// The loop body of three_tier.py:809-832 is a chain of four dependent [B,D] products per audio sample
// (embedding gather-sum -> L2 -> L3 -> Output -> argmax -> next sample).  As separate launches each link costs a
// launch (~6 us: 31.7 us per sample at B = 32, D = 1024); as phases of a chip-wide persistent kernel each link costs a
// cross-XCD hand-off (~4.7 us).  But the streams are independent and the sample-level MLP is small, so the
// chip is split along its XCDs instead: XCD x (32 CUs, one workgroup each, private L2) runs streams 4x .. 4x+3 through
// the complete MLP, and nothing ever crosses an XCD boundary:
//   * the first product of the chain is gone (round 5): everything in front of L2's ReLU is linear, so the caller
//     composes it through W2 -- the embedding tables (t2tbl[pos] = emb_tbl[pos] . W2) and the frame tier's output
//     projection (frame_out = h . (Wout_i . W2) + bout_i . W2 + b2) -- and L2's pre-activation is a ten-row gather-sum:
//     nine rows known a step early (summed in the shadow of the previous step), the newest sample's row from this CU's
//     slice of t2tbl[FS-1] in LDS (32 KB).  Per sample: three hand-offs and two products instead of four and three;
//   * every CU owns D/32 output columns of L3 and Q/32 of the output layer and keeps those weight slices in VGPRs
//     (64 + 16 per thread) for the whole launch: no weight traffic per sample;
//   * a hand-off = 16-byte stores of the CU's [4 streams x columns] slice (write-through into the XCD's L2) and sc1
//     loads (TCP miss, L2 hit) on the consumer side that re-read a slot until it is no longer EMPTY (a NaN payload):
//     one store-to-load latency per link.  The counted variant (store, s_waitcnt, L2 atomic, poll, load) measured
//     1.66 us in isolation (tools/xcd_probe.hip; agent-scope fences: 45 us, buffer_inv: 15 us) and 4 us per link inside
//     this kernel, of which 2.4 us were the four serialised L2 round trips;
//   * the 4 streams of a team ride in the 4 lanes of an f32x4, the products run on the vector ALUs (a 4-row tile wastes
//     3/4 of an MFMA; v_pk_fma_f32 has the same f32 peak as the matrix pipe);
//   * the pick (argmax with lowest-index ties, or the seeded inverse-CDF draw, among all codes, the top_k most likely, their
//     nucleus or the codes above the min-p bar: sr_common.h, srp_topk_keep, srp_topp_keep and srp_minp_keep) is recomputed by every CU of the team from
//     the team's logits, so the new sample index is local knowledge everywhere and the embedding gather of the next step
//     needs no further hand-off.
// One launch covers the FRAME_SIZE steps between two frame-tier steps; the tiers above stay on the launch path.
// Every spin is bounded; a team that times out (or a workgroup that finds its XCD's team already complete) raises the
// abort word, everybody leaves, srp_status() reports it and the caller falls back to the per-sample launches.
#include "sr_persist.h"

#include <stdlib.h>

#include "sr_common.h"
#include "switches.h"

namespace {

// -DSRP_FINE_TIMERS: step 5 of a timed launch also stamps the inside of its two products (tools/sr_timing.py)
#ifdef SRP_FINE_TIMERS
#define SRP_FINE(slot) (timing && i == 5 ? stamps + (slot) : nullptr)
#else
#define SRP_FINE(slot) nullptr
#endif

// MG = true (SrpArgs::ngroups > 1): the launch takes the batch in ngroups row groups of SRP_ROWS * SRP_NTEAMS = 32 streams,
// one after the other; group grp's team `team` runs streams (grp * SRP_NTEAMS + team) * SRP_ROWS + 0 .. 3.  What a launch
// pays for once does not depend on the streams and is loaded in front of the group loop -- the census atomic, the table
// slice in LDS, the W3 / W4 slices in registers, the biases --; what does (carry, history, gather, the sample steps, the
// tail) is the body of the loop, with exchange slots and a carry of its own per (group, team), so the slot life cycle
// below holds per group.  MG = false is the one-group kernel, instruction for instruction what it was before the loop
// existed (srp_launch takes it whenever ngroups == 1); profiles/samplernn_groups_kernel_resources.txt has both sets.
//
// FX = true (srp_fx_kernel<D, MG>, taken when SrpArgs::forced, SrpArgs::logp or SrpArgs::dlogp is set): the body that can take
// a step's sample from the caller, that writes the log-probability of every sample and that writes what every step drew from.  Kernels of their own, not branches of the
// one kernel: FX = false (srp_kernel<D, MG>, under the name it always had) compiles no line of either facility, so a plan
// that uses neither runs the step loop it ran before they existed (the sequential walk has measured 1.9 us per step slower
// for one store added in front of the loop: the top-p record), and srp_kernel<1024, true>, which already spills, is not asked
// for another scalar across its loop -- srp_fx_kernel<1024, true> is, and spills thirteen VGPRs where that one spills three
// (profiles/samplernn_forced_kernel_resources.txt, profiles/samplernn_min_p_kernel_resources.txt).  Inside FX = true the
// three are uniform branches.  The forced codes are
// team-local knowledge like the pick they replace: the prologue parks the launch's nsteps codes of the group's rows in the
// shared block (anything outside 0 .. Q-1 as -1 = free), as it parks the per-utterance entries, and the step chain reads
// them from there -- no global load in it.  The body is sr_persist_body.h, included once per kernel name.
#define SRP_KERNEL srp_kernel
#define SRP_FX false
#include "sr_persist_body.h"
#undef SRP_KERNEL
#undef SRP_FX
#define SRP_KERNEL srp_fx_kernel
#define SRP_FX true
#include "sr_persist_body.h"
#undef SRP_KERNEL
#undef SRP_FX

size_t srp_lds_bytes(int D) {
    return (size_t)(D + 256 + SRP_Q) * 16 + (size_t)(4 * SRP_Q + 4 * (D / 32) + SRP_Q * (D / 32)) * 4 + sizeof(SrpShared) + 64;
}

}  // namespace

int srp_max_groups() {
    const int g = env_int("PARROT_SR_PERSIST_GROUPS", 1);
    return g < 1 ? 1 : g > SRP_MAXGROUPS ? SRP_MAXGROUPS : g;
}

int srp_groups_for(int B, int max_groups) {
    const int mg = max_groups < 1 ? 1 : max_groups > SRP_MAXGROUPS ? SRP_MAXGROUPS : max_groups;
    constexpr int per = SRP_ROWS * SRP_NTEAMS;
    return B >= 1 && B <= per * mg ? (B + per - 1) / per : 0;
}

bool srp_eligible(int B, int D, int Q, int FS, int max_groups) {
    static int cus = -1;
    const int enabled = env_int("PARROT_SR_PERSIST", 1);
    if (cus < 0) {
        hipDeviceProp_t prop;
        int dev = 0;
        cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 0;
    }
    if (!enabled || cus != SRP_TEAM * SRP_NTEAMS) return false;
    if (srp_groups_for(B, max_groups) == 0 || Q != SRP_Q || FS < 1 || 2 * FS > SRP_MAXHIST) return false;
    return D == 256 || D == 512 || D == 1024;
}

long long srp_ws_floats(int D, int Q, int groups) {
    return srp_carry_base(D, Q, groups) + (long long)groups * SRP_NTEAMS * SRP_CARRY_WORDS;
}

int srp_init_ws(float* ws, int D, int Q, int groups) {
    // barrier / census / abort words zero, every hand-off slot EMPTY
    PH_CHECK(hipMemset(ws, 0, SRP_SYNC_WORDS * sizeof(float)));
    PH_CHECK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(ws + SRP_SYNC_WORDS), (int)SRP_EMPTY,
                          (size_t)groups * SRP_NTEAMS * srp_team_vecs(D, Q) * 4));
    // no carry yet: the sample index it is for can never match
    PH_CHECK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(ws + srp_carry_base(D, Q, groups)), -1,
                          (size_t)groups * SRP_NTEAMS * SRP_CARRY_WORDS));
    return (int)hipDeviceSynchronize();
}

SrpCarryKeys srp_carry_keys(float* ws, int D, int Q, int groups) {
    SrpCarryKeys k;
    k.key0 = ws ? reinterpret_cast<int*>(ws + srp_carry_base(D, Q, groups)) : nullptr;
    k.stride = SRP_CARRY_WORDS;
    k.rows = SRP_ROWS;
    k.blocks = groups * SRP_NTEAMS;
    return k;
}

int srp_status(const float* ws) {
    unsigned w[2] = {0, 0};
    if (hipMemcpy(w, reinterpret_cast<const unsigned*>(ws) + 512, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return w[0] ? (int)(w[1] ? w[1] : 1) : 0;
}

namespace {

template <int D>
int srp_prepare_width(int lds) {
    PH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(srp_kernel<D, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    PH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(srp_kernel<D, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    PH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(srp_fx_kernel<D, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    PH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(srp_fx_kernel<D, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return 0;
}

// one group: the kernel without the group loop, whatever the switch says; forced samples or log-probabilities: the
// instantiations that know them, and only then
template <int D>
void srp_launch_width(const SrpArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
    const bool fx = a.forced || a.logp || a.dlogp;
    if (a.ngroups > 1 && fx) hipLaunchKernelGGL((srp_fx_kernel<D, true>), grid, block, lds, stream, a);
    else if (a.ngroups > 1) hipLaunchKernelGGL((srp_kernel<D, true>), grid, block, lds, stream, a);
    else if (fx) hipLaunchKernelGGL((srp_fx_kernel<D, false>), grid, block, lds, stream, a);
    else hipLaunchKernelGGL((srp_kernel<D, false>), grid, block, lds, stream, a);
}

}  // namespace

int srp_prepare(int D) {
    const int lds = (int)srp_lds_bytes(D);
    switch (D) {
        case 256: return srp_prepare_width<256>(lds);
        case 512: return srp_prepare_width<512>(lds);
        case 1024: return srp_prepare_width<1024>(lds);
        default: return PH_ERR_UNSUPPORTED;
    }
}

int srp_launch(const SrpArgs& a, hipStream_t stream) {
    if (!a.ws || !a.origin || a.nsteps < 1 || a.FS + a.nsteps > SRP_MAXHIST) return PH_ERR_BADARG;
    if (a.ngroups < 1 || a.ngroups > SRP_MAXGROUPS || a.B < 1 || a.B > SRP_ROWS * SRP_NTEAMS * a.ngroups) return PH_ERR_BADARG;
    const size_t lds = srp_lds_bytes(a.D);
    const dim3 grid(SRP_TEAM * SRP_NTEAMS), block(SRP_THREADS);
    switch (a.D) {
        case 256: srp_launch_width<256>(a, grid, block, lds, stream); break;
        case 512: srp_launch_width<512>(a, grid, block, lds, stream); break;
        case 1024: srp_launch_width<1024>(a, grid, block, lds, stream); break;
        default: return PH_ERR_UNSUPPORTED;
    }
    return (int)hipGetLastError();
}

// Persistent-thread sample-level kernel of the SampleRNN generation loop (three_tier.py:452-515, 809-832): all
// FRAME_SIZE sample steps between two frame-tier steps in ONE launch.  See sr_persist.hip.
#pragma once
#include "common.h"

// Per-utterance draws (samplernn_generate_set_utterance_draws): one entry per stream, owned by the plan.  With the
// entries in force the seeded draw of buffer index t in stream b hashes seed ^ K1 (origin + t - off + 1) -- no stream
// term --, where off is the run index (origin + buffer index) of the first sample of the utterance's Q/2 prefix slot: the
// counter is the sample's index in the utterance's own buffer, wherever the utterance sits.  temperature <= 0: argmax.
// top_k: the utterance's truncation (samplernn_generate_set_utterance_top_k; the plan's without); outside 1 .. Q-1: none.
// top_p: its nucleus (samplernn_generate_set_utterance_top_p; the plan's without); not strictly between 0 and 1: none.
// min_p: its min-p bar (samplernn_generate_set_utterance_min_p; the plan's without); outside (0, 1]: none.
struct SrUttDraw {
    unsigned long long seed, off;
    float temperature; int top_k;
    float top_p; float min_p;
};
static_assert(sizeof(SrUttDraw) == 32, "the kernels read an entry's fields at fixed byte offsets");

struct SrpArgs {
    const int* tbase; int toff;        // first sample index of this launch: tbase[0] + toff
    int* samples; int len;             // [B][len] sample history (read: the FS samples before t0; written: t0 .. t0+nsteps-1)
    int B, D, Q, FS, nsteps;
    // Everything in front of L2's ReLU composed through W2 by the plan (samplernn.hip, SrPlan::make_composed):
    const float* t2tbl;                // [FS][Q][D] = emb_tbl[pos] . W2 (Embedding folded with L1_PrevSamples, then with L2)
    const float* frame_out; int ldf;   // [B][ldf]; step i adds columns [i*D, (i+1)*D) of h . (Wout . W2) + bout . W2 + b2
    const float* W3; const float* b3;  // [D][D], [D]
    const float* W4; const float* b4;  // [D][Q], [Q]
    float* logits;                     // [B][Q]: logits of the launch's last step (or null)
    // Optional: the frame tier's input for the NEXT frame (three_tier.py:398-411), computed by every team for its own
    // streams from the samples it has just produced: next_in[b][d] = next_bias[d] + next_add[b][d] + sum_i xf_i * next_Win[i][d],
    // xf_i = (sample / (Q/2) - 1) * 2 of the launch's last FS samples.  next_in == null: not computed.
    // Round 5: next_n (0 = D) is the width of that product -- with next_Win = Win . U ([FS, 3D], composed by the plan) and
    // next_add = the big-tier share of the pre-activations, the kernel leaves the frame tier's additive gate / candidate
    // inputs themselves ([B, 3D]) and the tier's two step GEMMs walk K = D instead of 2 D.  next_bias may be null.
    float* next_in; const float* next_Win; const float* next_bias; const float* next_add; int next_ld_add, next_n;
    // With next_n = 3 D and next_gpre = h . Wg of the next frame ([B, 2D], update | reset: made beside the output projection,
    // it does not depend on the new samples) the kernel also finishes that frame's gates: next_z = sigm(gpre_z + in_z),
    // next_rh = sigm(gpre_r + in_r) * next_h; only the candidate's third of next_in is written.  Null: not computed.
    const float* next_gpre; const float* next_h; float* next_z; float* next_rh;
    float* ws;                         // srp_ws_floats() floats, prepared once by srp_init_ws
    float temperature; int pad;
    unsigned long long seed;
    int ngroups;                       // row groups of 32 streams this launch takes one after the other: ceil(B / 32), the
                                       // count ws was sized and initialised for (1: the kernel without the group loop)
    // Draw origin (device word, required): the seeded draw of sample index t is keyed by origin[0] + t -- 0 in a run of one
    // piece; a resumed segment (samplernn.hip, sr_resume_kernel) counts the samples the ring has turned past in it.
    const unsigned long long* origin;
    // Per-utterance draws: [B] entries, or null = the plan's key (seed, stream) and temperature above.  Wave r picks for
    // row srow + r, so its entry is wave-uniform: fetched once per launch and row group into the shared block.
    const SrUttDraw* utt;
    // SampleRnnGenDesc::draw_mode: 0 = one lane walks the codes (the default's bits), 1 = the wave-parallel draw
    // (sr_common.h, srp_scan_draw).  A uniform branch of the pick, like utt.
    int draw_mode;
    // SampleRnnGenDesc::top_k: a draw at temperature > 0 is taken among the k most likely codes (sr_common.h, srp_topk_keep);
    // 0: among all of them, by the instructions of the pick without this field.  With utt: the entry's top_k.  The launcher
    // hands the kernel 0 for a value outside 1 .. Q-1, and sets SRP_NUCLEUS beside it when top_p is active and SRP_MINP when
    // min_p is: one word for the pick to test (srp_trunc_word).
    int top_k;
    // samplernn_generate_set_top_p: a draw at temperature > 0 is taken among the nucleus of the codes top_k left (sr_common.h,
    // srp_topp_keep); active strictly between 0 and 1 (top_k then carries SRP_NUCLEUS).  With utt: the entry's top_p.
    float top_p;
    // samplernn_generate_set_min_p: of the codes both left, a draw keeps those whose term is >= min_p (sr_common.h,
    // srp_minp_keep); active in (0, 1] (top_k then carries SRP_MINP).  With utt: the entry's min_p.
    float min_p;
    // samplernn_generate_set_forced: [B][len] like samples, or null.  Where forced[b][t] is a code in 0 .. Q-1 the step at
    // buffer index t of stream b computes its logits and its pick as always and then takes that code as the sample -- into
    // samples, the history of the following steps, the carry and the next frame's input; any other value (-1): the pick.
    // A forced step consumes no uniform: the draw counter is the sample's index.
    const int* forced;
    // samplernn_generate_set_log_probs: [B][len] like samples, or null.  Every step writes the natural logarithm of the
    // model's probability (temperature 1, no truncation) of the sample it wrote: logits[s] - max - log(sum exp(logits - max)).
    float* logp;
    // samplernn_generate_set_draw_stats: [B][len] both like samples, or both null.  Every step writes kept = the size of the
    // set its pick was drawn from (1 on an argmax step, Q on an untruncated draw) and dlogp = the natural logarithm of the
    // probability of the sample it wrote under the distribution it drew from: (logits[s] - max) / T - log(sum of the kept
    // terms), -inf for a sample outside the kept set (a forced one), 0 for the argmax on an argmax step.
    float* dlogp; int* kept;
};

constexpr int SRP_NUCLEUS = 1 << 16;  // in SrpArgs::top_k: the plan's top_p is active
constexpr int SRP_MINP = 1 << 17;     // ... and its min_p
inline int srp_trunc_word(int top_k, float top_p, float min_p, int Q) {
    return (top_k > 0 && top_k < Q ? top_k : 0) | (top_p > 0.f && top_p < 1.f ? SRP_NUCLEUS : 0) |
           (min_p > 0.f && min_p <= 1.f ? SRP_MINP : 0);
}

// PARROT_SR_PERSIST_GROUPS (switches.h): the largest number of row groups a launch may take, clamped to 1 .. 8
int srp_max_groups();
// Row groups a batch of B streams takes, ceil(B / 32), or 0 when that is more than max_groups (clamped to 1 .. 8) or
// B < 1.  No device needed.
int srp_groups_for(int B, int max_groups);
bool srp_eligible(int B, int D, int Q, int FS, int max_groups);
// sync words + groups * 8 exchange blocks + groups * 8 carries; with one group every offset is the one-group kernel's
long long srp_ws_floats(int D, int Q, int groups);
int srp_init_ws(float* ws, int D, int Q, int groups);  // once per plan: sync words zero, hand-off slots EMPTY
int srp_prepare(int D);  // once per process and width, outside stream capture (raises the kernel's LDS limit)
int srp_launch(const SrpArgs& a, hipStream_t stream);
// 0 when no launch on this workspace has timed out / mis-teamed so far
int srp_status(const float* ws);

// The launch-to-launch carry (sr_persist.hip, prologue) as seen from outside the kernel: the word that holds the sample
// index a carry block is for, per block, and the streams a block serves.  A kernel that rewrites the sample history of
// stream b behind the sample kernel's back (an utterance start inside a packed run, samplernn.hip) invalidates the
// carry of b's team -- the state srp_init_ws leaves -- and the next sample launch walks the chain from `samples` for all
// rows of that team, as the first launch of any utterance does.
struct SrpCarryKeys {
    int* key0;   // key word of block 0 (null: no persistent kernel)
    int stride;  // words from one block's key to the next one's
    int rows;    // stream b belongs to block b / rows (blocks are numbered group * teams + team)
    int blocks;  // blocks in all (groups * teams)
};
SrpCarryKeys srp_carry_keys(float* ws, int D, int Q, int groups);
__device__ inline void srp_carry_invalidate(const SrpCarryKeys& k, int b) { k.key0[(size_t)(b / k.rows) * k.stride] = -1; }

// Persistent phase machine: the decoder scan as ONE resident kernel (gfx950).
//
// Replaces the thousands of per-step launches of the wavefront schedules (plans.hip) for the scan of
// Parrot.compute_cost (reference model.py:651-737).  One workgroup per CU stays resident for the whole window; a
// tick = n_slots phases separated by grid barriers; in a phase every workgroup runs up to maxu work units from a
// host-built table.  A unit is a 16-column tile of a recurrent-step GEMM over all batch rows with the GRU gate math
// (decode: or the LSTM cell update) fused (the same algebra as sk_kernel's epilogues, Blocks GatedRecurrent /
// sampleRNN/lib/ops.py:364-393), or the
// GMM-window attention of one batch row (model.py:664-690).  What the launches could not do:
//   * weights are STATIONARY: a unit's [K,16] weight slab is copied into the CU's LDS once per window (up to 144 KB per
//     CU) and every step reads it from there; only what does not fit is streamed from the fragment-major copies;
//   * activations travel between workgroups in fragment-major slabs (1 KB blocks in MFMA operand order), stored
//     write-through (sc1) by the producing epilogue and read with sc1 loads by the consumers, so the only inter-phase
//     cost is the barrier (XCD-hierarchical, ~2.4 us measured, tools/persist_probe.hip) -- no launch, no cold start;
//   * the projections of lower-layer outputs into a layer (Fork h{j}_to_h{l}, inp_to_h{l}; model.py:692-722) run as
//     separate units one tick ahead of the layer's recurrent units, so every phase's longest dependent GEMM has
//     K = H instead of K = (l+1) H + E.
#pragma once
#include "common.h"

enum { PM_MAXENT = 12,   // unit descriptors per workgroup: n_slots * maxu <= PM_MAXENT (training 3 x 3, decode 9 x 1)
       PM_MAXSLOTS = 9, PM_THREADS = 512, PM_MAXINIT = 12, PM_MAXDST = 6, PM_MAXWDST = 8, PM_MAXFILL = 16 };
// PM_GEMM16: a GEMM unit whose weight slab is a bf16 copy (decode with bf16 operands, below); every other field as PM_GEMM
// PM_SAMPLE: the GMM head's sampling of one batch row (decode, PmSamp below); row = the batch row, dst[] = the fed-back-frame
// chunks of the layer slabs of the NEXT step (off already points at them, as PmAtt::wdst)
enum { PM_NONE = 0, PM_GEMM = 1, PM_ATT = 2, PM_GEMM16 = 3, PM_SAMPLE = 4 };
enum { PM_EPI_LINEAR = 0, PM_EPI_GATES = 1, PM_EPI_CAND = 2, PM_EPI_LSTM = 3 };

// LDS map (floats): resident weights | scratch shared by the split-K reduction (8 partial 16x16 tiles, rows padded
// to 20 floats) and the attention row (never live at the same time) | the workgroup's unit table | misc.
enum {
    PM_LDS_W = 36864,                 // 144 KB = 2304 K-rows of a 16-column tile
    PM_LDS_RED = 8 * 16 * 20,         // 10 KB
    PM_LDS_UNITS = 1280,              // 5 KB: PM_MAXENT unit descriptors
    PM_LDS_MISC = 64,                 // census, flags, phase timers
    PM_LDS_FLOATS = PM_LDS_W + PM_LDS_RED + PM_LDS_UNITS + PM_LDS_MISC,
    PM_ATT_MAXU = 800,                // context length limit of the in-kernel attention (208 + U + 512 + 512 floats <= PM_LDS_RED)
    PM_ATT_MAXA = 32,
};

// Row-major operand at step t: p + t * st (floats), leading dimension ld; p already points at the unit's first column.
struct PmRM {
    float* p;
    long long st;
    int ld, pad;
};

// Fragment-major activation slab of one step: [MB row blocks][K/16 chunks][256 floats]; block (rb, c) holds, for lane
// l = kk*16 + r, the four values X[16 rb + r][16 c + 4 kk + 0..3] -- the A operand of four 16x16x4 MFMAs.
// Every unit reads ONE slab (its whole K range, e.g. [h0[t] ; w[t]] for the layer-0 gates): the producers write their
// tiles into every slab that contains them (PmDst), so the consumer's K loop needs no segment lookup.
// Slabs are addressed as BYTE offsets from PmProgram::fm_base (one buffer resource for the whole region, < 4 GB).
struct PmDst {
    unsigned off, st;   // slab of step t = fm_base + off + t * st
    int nch, chunk;     // chunks per row block of that slab / chunk of the producer's first column
};

struct PmUnit {
    int kind, lag, K, w_lds;     // w_lds >= 0: float offset of the resident weight slab in LDS; -1: stream from W
    unsigned a_off, a_st;        // the activation slab the unit reads
    int a_nch, a_c0;             // chunks per row block of that slab / the unit's first chunk in it (K/16 chunks are read)
    const float* W;              // fragment-major weights of the unit: [K/16][256] floats (PM_GEMM16: [K/32][512] bf16)
    int epi, M, rtile, row;      // rtile: GATES tile of the reset gate (LSTM: the tile's quarter of a block, below; LINEAR: 1 + the
                                 // frame's column tile on the unit a forced program selects in, PmForce); row: batch row of an ATT unit
    const float* bias;           // 16 floats (the tile's columns) or null
    PmRM add[4];                 // additive pre-activation inputs (p == null: unused)
    PmRM e0, e1;                 // GATES (r tile): e0 = h_prev;  CAND: e0 = h_prev, e1 = z
    PmRM out, o1, o2;            // LINEAR: out;  GATES: o1 = z | o2 = r, out = r*h_prev;  CAND: o1 = c, out = h_new
    int ndst, gstr;              // fragment-major copies of `out` for the consuming units; gstr: LSTM gate stride (H)
    PmDst dst[PM_MAXDST];
    // LSTM (decode): the unit's 16 columns are 4 hidden units x 4 gates in sk_col order (column 4 q + j = gate q of hidden
    // unit 4 ct + j; i | f | o | g), its weights the tile ct of parrot_tile_weights(.., lstm_H = H).  bias / add[] stay in
    // the natural gate-major order [4H] and point at column 4 ct: the finalising lane (kk, r16) holds gate kk and reads its
    // quad at + kk * gstr.  e1 = c_prev, o1 = c_new, out = h_new (row-major, ld H, pointing at column 4 ct; both
    // write-through).  The tile yields FOUR state columns = the 16 lanes kk' = rtile (= ct % 4) of block dst[].chunk
    // (= first chunk of h in the slab + ct / 4): four units complete one fragment-major block.
    // Round 5 (decode, batch <= 16): the attention projection folded into layer 0's candidate units.  pw[jt] = the
    // fragment-major block of the padded projection matrix Watt [H, 32] for this unit's 16 state columns and output
    // column tile jt; the finalising wave multiplies the h_new tile it holds by them (8 MFMAs) and publishes the
    // [B, 32] partial sums at pp (row-major, write-through) -- the attention row then adds H / 16 partials of 32 values
    // instead of reading its state row and the 120 KB projection matrix.  pw[0] == null: no fold.
    const float* pw[2];
    PmRM pp;
    // bf16 operands (decode, kind = PM_GEMM16; K a multiple of 32): the unit walks K in 32-deep steps.  Step s takes the two
    // f32 activation blocks 2s and 2s + 1 of its slab -- lane (kk, r) holds X[r][32 s + 4 kk .. + 3] and
    // X[r][32 s + 16 + 4 kk .. + 3] --, rounds them to bf16 (nearest even) where they enter the product and issues ONE
    // v_mfma_f32_16x16x32_bf16 against the 1 KB block s of W, whose lane (kk, n) holds the same eight K rows of column n
    // (parrot_tile_weights_bf16, mode 2): an MFMA does not care about a permutation of K both operands share, so no lane
    // moves anything.  The slabs stay f32 (the dataflow hand-off polls f32 slots BEFORE they are rounded), accumulation,
    // epilogue and outputs are those of the PM_GEMM unit.  A resident slab takes K * 8 floats of LDS instead of K * 16.
};

struct PmAtt {
    PmRM h1;                      // layer-0 state history [T+1,B,H]: row-major, p = slot 0
    const float* WattT; const float* batt; const float* ctx;
    float* kappa;                 // [T+1,B,A]
    float* a; float* b;           // [T,B,A]
    float* phi;                   // [T,B,U]
    float* w;                     // [T+1,B,E] row-major
    int nwdst, pad3;              // fragment-major copies of w[t+1] (slab of step t+1 for layer 0, step t above)
    PmDst wdst[PM_MAXWDST];       // off already points at the slab the value of step t goes to (t * st is added)
    int* sup;                     // [T,B,2] or null
    const float* pp;              // (round 5) per-tile partial sums of the projection, [T][H / 16][B][32], or null
    long long pp_st;              // floats per step
    int B, H, A, U, E, att_type, dense, pad;
    float eps, alignment, sharpening, timing;
    // Optional end-of-utterance stop (decode, ParrotSampleDesc::eou_*; all null / 0: the launch runs every tick).  Row b's
    // predicate at step t is phi[t, b, eou_pos[b]] > phi[t, b, j] for all j < eou_ncmp[b] (strict; NaN never holds; no j:
    // holds), evaluated on the row's phi in LDS.  eou_first[b] = the first step it held, or -1 (reset by pm_launch).
    // Once every row has fired, the launch ends after frame max_b min(T, eou_first[b] + eou_extra) -- see pm_kernel.
    const int* eou_pos; const int* eou_ncmp;
    int* eou_first;
    int eou_extra, pad4;
};

// GMM head on the machine (decode, ParrotSampleDesc::gmm_K > 0; K == 0: the program has no sampling units).  The head
// phase -- plain LINEAR units over the composed matrix Wr . [W_mu | W_sig | W_co] -- leaves the row-major, write-once head
// history head[t] = [B, NH] (NH a multiple of 16: mu at column o K + k, sig_hat at O K + o K + k, the mixture logits at
// 2 O K + k); the PM_SAMPLE unit of row b then does gmm_sample_kernel's arithmetic (elementwise.hip) with one wave: mixture
// weights, the pick against unif[t, b], x[t + 1] = mu + (exp(sig_hat - bias) + eps) noise[t, b, :], stored row-major
// (64 columns, zeros from O on) and as 16 fragment-major quads into every PmUnit::dst.
struct PmSamp {
    PmRM head;                    // p = step 0, st = B * NH, ld = NH
    const float* unif;            // [T, B]
    const float* noise;           // [T, B, O]
    float* x;                     // row-major frame of step 0's OUTPUT (= slot 1 of ParrotSampleDesc::x), [.., B, ldx]
    float* pi;                    // [T, B, K]
    int B, O, K, ldx;
    float bias, eps;
};

struct PmInit {  // prologue: row-major [M,K] (ld) -> chunks [chunk, chunk + K/16) of a fragment-major slab
    const float* src;
    unsigned dst_off;
    int nch, chunk, ld, K, pad;
};

// Dataflow mode (PmProgram::dataflow): no grid barriers.  Every buffer a unit reads from another workgroup is write-once
// per launch; pm_launch fills those buffers (PmFill) with PM_EMPTY, a NaN payload arithmetic never produces, producers
// overwrite 16-byte slots with single write-through stores, and consumers re-read a slot until it is full.  A unit's
// inputs always come from units at earlier (tick, slot) positions and every workgroup walks its units in (tick, slot)
// order, so some unit can always run.  A hand-off then costs one store-to-load latency instead of store acknowledgement
// + barrier + load.
struct PmFill {
    void* p;
    long long bytes;
};

struct PmProgram {
    int T, n_ticks, nwg, MB, M, ninit, n_slots, maxu;  // a tick = n_slots phases of up to maxu units per workgroup
    int dataflow, nfill;
    int lstm, w16;        // lstm: some units are PM_EPI_LSTM (selects the kernels compiled with that epilogue); w16: some
                          // are PM_GEMM16 (the kernels that also carry the bf16 K loop; decode programs, LSTM or GRU)
    PmFill fill[PM_MAXFILL];
    const PmUnit* units;  // device: [n_slots][nwg][maxu]
    unsigned* sync;       // device: PM_SYNC_WORDS + PM_DBG_WORDS unsigned, zeroed before every launch
    float* fm_base;       // start of the fragment-major slab region (all PmDst / a_off offsets are relative to it)
    PmAtt att;
    PmInit init[PM_MAXINIT];
    PmSamp samp;          // (last: the programs without a GMM head keep the argument layout they had)
};

enum { PM_SYNC_WORDS = 1024, PM_DBG_WORDS = 256 * 24 * 2 };  // dbg: per workgroup 24 x u64: work[9], wait[9] per slot, 4 gemm stages (100 MHz ticks)
// word offsets inside `sync` (128 B apart)
enum { PM_S_XCNT = 0, PM_S_XGEN = 256, PM_S_TOP = 512, PM_S_CENSUS = 544, PM_S_TOTAL = 800, PM_S_ABORT = 832,
       // end-of-utterance stop (PmAtt::eou_*): the tick at which every workgroup leaves (0: none yet; written once), the
       // largest row length so far, the rows that have fired, the ticks the owner of attention row 0 executed
       PM_S_STOP = 864, PM_S_EOUMAX = 896, PM_S_EOUCNT = 928, PM_S_TICKS = 960,
       PM_S_STICKY = 992 };  // words >= PM_S_STICKY survive pm_launch's clearing: [PM_S_STICKY] != 0 = some launch gave up
// The smallest PmAtt::eou_extra a program may ask for.  The stop tick is published while some attention row works on step
// t_p, and is >= t_p + eou_extra + D (D = n_ticks - T, the largest lag).  A unit of step t' reads values that depend on
// every attention row of step t' - 3 or later (its newest operands are products of step t' - 1, theirs hold w[t' - 1] =
// the attention of step t' - 2; one more for slack), so a workgroup that owns units has started no tick beyond
// t_p + D + 3 when the word appears, its look at the word for the tick after that may already be under way (the look is
// asked for one tick ahead), and the first tick certain to see the word is t_p + D + 5 <= the stop tick for
// eou_extra >= 5.  8 leaves three ticks of margin.  With grid barriers every workgroup sees the word two ticks later.
enum { PM_EOU_MIN_EXTRA = 8 };
#define PM_EMPTY 0x7FC0DEADu

// Per-row decode controls (parrot_sample_set_row_controls): [B] device arrays that take the place of PmAtt::sharpening /
// PmAtt::timing and PmSamp::bias, row b reading element b.  A second kernel argument, not part of PmProgram: a program
// without them keeps its records and its digest, and the kernels launched without them (ROW = false) never read it.  With
// them all of timing / sharpening are set, and bias whenever the program has sampling units.
struct PmRows {
    const float* timing; const float* sharpening; const float* bias;
};

// Forced frames (decode, ParrotSampleForcedDesc::forced / n_forced / own_x): while t < n[b] the frame fed back into step t + 1 of
// row b is forced[t, b] instead of what the model emitted (MSE head) or drew (GMM head).  The unit that produces the frame
// does the select in its epilogue, in front of its stores: a LINEAR unit of a forced program whose PmUnit::rtile is 1 + ct
// owns columns 16 ct .. 16 ct + 15 of the frame (rtile is 0 on every other LINEAR unit and in every program without
// forcing); a PM_SAMPLE unit owns the whole row.  The value computed BEFORE the select goes to own_x[t, b] (row-major, a
// plain store: nothing inside the launch reads it); the selected value goes to x[t + 1] and to every PmDst copy, so a slab
// holds the bits the row-major frame holds.  Columns >= O of a forced frame are not read and are fed back as zero.  A
// third kernel argument, as PmRows is the second and for the same reason: a program without forcing keeps its records and
// its digest, and the kernels compiled without it (FRC = false) never read it.  The kernels with it always carry the row
// controls too (ROW = true): the forced launcher takes both.
struct PmForce {
    const float* forced;  // [T, B, ldx]
    const int* n;         // [B], 0 <= n[b] <= T
    float* own_x;         // [T, B, ldx]
    int B, O, ldx, pad;
};

int pm_launch(const PmProgram& prog, hipStream_t stream, const PmRows* rows = nullptr);
// the same launch with forced frames: the kernels of persist_forced.hip (f32 operands only: prog.w16 == 0)
int pm_launch_forced(const PmProgram& prog, hipStream_t stream, const PmRows& rows, const PmForce& force);
// synchronises; frames the last launch completed: T, or fewer when the end-of-utterance stop ended it (PmAtt::eou_extra > 0)
int pm_steps_run(const PmProgram& prog, int* steps);
int pm_status(const PmProgram& prog);  // synchronises; 0, or non-zero when a launch on this program's workspace gave up
int pm_max_workgroups();  // number of workgroups the machine runs with on this device (one per CU, <= 256)

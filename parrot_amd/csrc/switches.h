// Runtime switches: every environment variable the library (and its Python host) reads, and the one place the library
// reads them.  Integer switches parse like atoi (leading blanks and sign, then digits; anything else counts as 0) and
// take their default only when unset; parrot_amd/utils.py env_int is the same parser on the Python side.
//
// Read at: "load" = once per process; "plan" = at plan creation (parrot_decoder_create, parrot_sample_create,
// parrot_samplernn_create); "launch" = in the launch check, i.e. at graph capture for captured plans.  None of the plan /
// launch reads is cached: tests and bench.py --full change them between plans of one process.
//
// switch                   default  read     selects                                                         set by
// PARROT_GEMM_PRECISION    (bf16x3) load     f32 | 0: every batched product on the f32-input MFMA kernel;   development
//                                            bf16 | 1: plain bf16 operands; else split-bf16 (bf16x3).
//                                            Known issue: Python (ops.py) maps bf16 | 1 to bf16x3, not bf16
// PARROT_SCHEDULE          -1       plan     decoder scan schedule: 0 / 3 / 5 / 7, 4 = persistent forward     tests, tools
//                                            scan (opt-in); -1 = by shape.  Python allocates schedule 4's
//                                            workspace when it reads 4
// PARROT_CHUNK             0        plan     > 0: forward scan chunk length (else the plan's own)            tests
// PARROT_S5_WSTEP          1        plan     0: schedule 5 reads the upper layers' w rows in the attention  tests
//                                            launch (round-5 placement) instead of their own step jobs
// PARROT_BWD_HETERO        1        plan     0: no K-balanced backward tick (bwd8); Python then allocates    tests
//                                            no second / third accumulators
// PARROT_GRU_ROWWISE       1        plan     0: no row-wise GRU sequence kernel                              tests
// PARROT_RG_WAVES          8        plan     waves per 16-row block of the row-wise GRU sequence kernels:    tests, tools
//                                            4 or 8 (other values round down); same results, bit for bit
// PARROT_WK                1        plan,    wide step kernel: 0 never, 1 launches of >= 4096 output          tests
//                                   launch   columns, 2 whenever legal
// PARROT_ATT_DENSE         0        plan,    1: the attention reads every context row instead of walking    bench.py, tests
//                                   launch   its support (same result)
// PARROT_ATT_BWD_NARROW    1        launch   0: the attention backward row block always fetches and reduces  tests, tools
//                                            its full 16 context rows per wave (no narrow path for supports
//                                            of at most 64 rows; same result, bit for bit)
// PARROT_PM_DATAFLOW       0 / 1    plan     persistent machines: 1 = per-unit flags, 0 = grid barriers;    tests
//                                            default 1 for the sampling plan cut in pieces and the LSTM
//                                            sampling plan with one unit per workgroup, 0 otherwise
// PARROT_SAMPLE_PERSIST    1        plan     0: sampling without the persistent machine, GRU and LSTM        tests, tools
//                                            (Python: no workspace)
// PARROT_PM_PIECES         1        plan     0: the sampling machine's whole-K phases instead of pieces      tests, tools
//                                            (GRU; the LSTM plan is whole-K either way)
// PARROT_PM_ATTFOLD        1        plan     0: attention projection not folded into the candidate units     development
//                                            (Python: no folded matrix)
// PARROT_PM_FBC            1        plan     0: fed-back frame kept in the step's chain (Python: no          tests
//                                            appended rows)
// PARROT_PM_GMM            0        plan     1: GMM-head models decode on the sampling machine too (composed   tests, tools
//                                            head phase + sampling phase; GRU whole-K and LSTM programs).
//                                            Python prepares the composed head and lifts its refusals when 1
// PARROT_PM_GRU_BF16       0        plan     1: decode_dtype='bf16' / ParrotSampleDesc::bf16 also decodes GRU   tests, tools
//                                            stacks (bf16 layer units in both GRU programs; no attention fold,
//                                            no composed feedback rows).  Python lifts its GRU refusal when 1
// PARROT_PM_DUMP_PLAN      unset    plan,    set: print the sampling machine's pieces and the barrier words  development
//                                   failure  of a persistent launch that gave up
// PARROT_SR_PERSIST        1        plan     0: SampleRNN sampling without its persistent kernel             tests
// PARROT_SR_PERSIST_GROUPS 1        plan     largest number of 32-stream row groups one launch of SampleRNN's  tests, tools
//                                            persistent kernel may take (1 .. 8, clamped): batches up to 32 x
//                                            this many streams leave the launch path.  Python sizes the
//                                            workspace through the library (samplernn_persist_floats)
// PARROT_SR_TIMING         0        load     SampleRNN persistent kernel's in-kernel timers                  tools
// PARROT_TRACE_ONLY        unset    plan     set: plans build on a machine without a GPU (schedule tracing)  tests, tools
//
// Python only (parrot_amd/):
// PARROT_WS_CACHE          6        alloc    workspace / plan cache entries per shape (at least 4)           development
// PARROT_READOUT_COMPOSED  1        step     0: readouts and output layer as separate full-width products    tests, tools
//                                            (the path of GMM / layer_norm / speaker / bf16 models anyway)
// PARROT_ENCODER_TABLES    1        step     0: the encoder's Fork products on the embedded text instead of   tests, tools
//                                            lookups in projected label tables (the path of tables taller
//                                            than 64 rows anyway)
// PARROT_GMM_COST_FUSED    1        step     0: GMM head cost and gradient as torch element-wise code         tests, tools
//                                            (the path of raw_output and k_gmm > 64 models anyway)
// PARROT_BF16_DW           1        step     0: bf16 decoders' weight gradients from f32 operands            tests
// PARROT_BF16_READOUT      1        step     0: bf16 decoders' readout stack on f32 operands                 tests, tools
// PARROT_BF16_DG16         1        alloc    0: LSTM backward scan leaves f32 pre-activation gradients       tools
// PARROT_SR_SKIP_STACKS    0        call     1: SampleRNN's device-resident generator takes skip-connection  tests, tools
//                                            stacks (SKIP_CONN, N_RNN >= 2): Python gathers the +inpskip /
//                                            outskip parameters and calls samplernn_generate_set_skip_stacks;
//                                            0: refused, generate_and_save_samples runs the literal loop.
//                                            The library itself does not read it: the setter is the switch
// PARROT_SKIP_INDEX_CHECK  0        import   1: embedding index bounds are not checked on the host           development
// PARROT_DP_BUCKETS        1        Trainer  0: gradient all-reduce in one bucket                            development
// PARROT_ALLREDUCE_BF16    0        Trainer  1: bf16 on the wire                                             development
// PARROT_DIST_FORCE        0        init     1: a one-rank process group counts as distributed               tests
// PARROT_DIST_BACKEND      (auto)   init     torch.distributed backend (string)                              bench.py, tests
// PARROT_HIP_LIB           (built)  load     path of an alternative build of the library (string)            tools
// PARROT_BUILD_TAG / _FLAGS, PARROT_PM_DEPTH   build    variant libraries / the machine's ring depth (parrot_amd/build.py)
#pragma once
#include <stdlib.h>

static inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
static inline bool env_set(const char* name) { return getenv(name) != nullptr; }
static inline const char* env_str(const char* name) { return getenv(name); }

// Switches read in more than one place.
static inline int sw_att_dense() { return env_int("PARROT_ATT_DENSE", 0); }
static inline int sw_att_bwd_narrow() { return env_int("PARROT_ATT_BWD_NARROW", 1) != 0; }
static inline int sw_pm_dataflow(int dflt) { return env_int("PARROT_PM_DATAFLOW", dflt); }
static inline int sw_rg_waves() { return env_int("PARROT_RG_WAVES", 8); }
static inline int sw_wk() { return env_int("PARROT_WK", 1); }
static inline bool sw_pm_dump_plan() { return env_set("PARROT_PM_DUMP_PLAN"); }

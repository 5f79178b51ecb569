// Host-side scan orchestration: the loops that theano.scan ran inside one theano.function call in
// the reference (model.py:726-737, 1038-1057; ops.py:299-327) become fixed launch sequences of the
// fused step kernels, captured once into a hipGraph and replayed per window (all pointers in a
// plan are fixed, so a replay costs one hipGraphLaunch instead of thousands of host launches).
#include "pm_builder.h"
#include "switches.h"

namespace {

// ----------------------------------------------------------------------------- GRU scan
struct GruSeqPlan : PlanBase {
    ParrotGruSeqDesc d;

    // Narrow layers (H <= 128, a multiple of 16: the encoder) run the whole sequence as ONE launch per direction on the
    // row-owning kernels of rowgru.hip (PARROT_GRU_ROWWISE=0: the per-step launches below).  The plan owns the fragment-major
    // weight copies and refreshes them at the head of every forward scan (the weights change between steps).
    bool rowwise = false;
    int reason = PARROT_GRU_ROUTE_SHAPE;  // why not row-wise (parrot_gru_seq_route); 0 when row-wise
    int waves = 4;           // PARROT_RG_WAVES, read with the plan
    float* tiled = nullptr;  // per chain: Wg_f, Wc_f, Wg_r, Wc_r
    ~GruSeqPlan() override {
        if (tiled) (void)hipFree(tiled);
    }
    int launch_path(int why) {  // the per-step launches, for this reason
        rowwise = false;
        reason = why;
        return 0;
    }
    int setup_rowwise() {
        if (!rowgru_supported(d.T, d.B, d.H, d.nchain)) return launch_path(PARROT_GRU_ROUTE_SHAPE);
        if (env_int("PARROT_GRU_ROWWISE", 1) == 0) return launch_path(PARROT_GRU_ROUTE_SWITCH);
        for (int ch = 0; ch < d.nchain; ++ch)  // (the tiling kernel wants 16-byte aligned matrices)
            if (!d.Wg[ch] || !d.Wc[ch] || ((uintptr_t)d.Wg[ch] & 15) || ((uintptr_t)d.Wc[ch] & 15))
                return launch_path(PARROT_GRU_ROUTE_UNALIGNED);
        waves = rowgru_waves(sw_rg_waves());
        const size_t per = (size_t)6 * d.H * d.H;  // 2 x (H x 2H + H x H) floats
        if (hipMalloc(&tiled, sizeof(float) * per * d.nchain) != hipSuccess) {
            tiled = nullptr;
            return launch_path(PARROT_GRU_ROUTE_ALLOC);
        }
        rowwise = true;
        reason = PARROT_GRU_ROUTE_ROWWISE;
        return 0;
    }
    RowGruArgs row_args() const {
        RowGruArgs g;
        memset(&g, 0, sizeof(g));
        const size_t HH = (size_t)d.H * d.H;
        for (int ch = 0; ch < d.nchain; ++ch) {
            RowGruChain& c = g.chain[ch];
            float* base = tiled + (size_t)ch * 6 * HH;
            c.Wg_f = base; c.Wc_f = base + 2 * HH; c.Wg_r = base + 3 * HH; c.Wc_r = base + 5 * HH;
            c.inputs = d.inputs[ch]; c.gate_inputs = d.gate_inputs[ch];
            c.h = d.h[ch]; c.z = d.z[ch]; c.r = d.r[ch]; c.rh = d.rh[ch]; c.c = d.c[ch];
            c.dh = d.dh[ch]; c.dG = d.dG[ch]; c.dC = d.dC[ch];
            c.reverse = d.reverse[ch];
        }
        g.mask = d.mask; g.T = d.T; g.B = d.B; g.H = d.H; g.nchain = d.nchain; g.waves = waves;
        return g;
    }
    int fwd_rowwise(hipStream_t st) {
        const RowGruArgs g = row_args();
        for (int ch = 0; ch < d.nchain; ++ch) {
            const RowGruChain& c = g.chain[ch];
            PL_TRY(sk_tile_weights_launch(d.Wg[ch], d.H, 2 * d.H, 2 * d.H, const_cast<float*>(c.Wg_f), 0, 0, st));
            PL_TRY(sk_tile_weights_launch(d.Wc[ch], d.H, d.H, d.H, const_cast<float*>(c.Wc_f), 0, 0, st));
            PL_TRY(sk_tile_weights_launch(d.Wg[ch], d.H, 2 * d.H, 2 * d.H, const_cast<float*>(c.Wg_r), 1, 0, st));
            PL_TRY(sk_tile_weights_launch(d.Wc[ch], d.H, d.H, d.H, const_cast<float*>(c.Wc_r), 1, 0, st));
        }
        return rowgru_fwd_launch(g, st);
    }

    int enqueue(int which, hipStream_t s) override {
        if (rowwise) return which == 0 ? fwd_rowwise(s) : rowgru_bwd_launch(row_args(), s);
        return which == 0 ? fwd(s) : bwd(s);
    }

    int fwd(hipStream_t st) {
        const size_t BH = (size_t)d.B * d.H;
        for (int s = 0; s < d.T; ++s) {
            SkJob jobs[4];
            for (int ch = 0; ch < d.nchain; ++ch) {
                const int t = d.reverse[ch] ? d.T - 1 - s : s;
                SkJob& j = jobs[ch];
                sk_gru_gates_job(j, d.B, d.H, d.h[ch] + s * BH, d.z[ch] + t * BH, d.r[ch] + t * BH, d.rh[ch] + t * BH);
                j.nseg = 1;
                j.seg[0] = sk_seg(d.h[ch] + s * BH, d.H, d.Wg[ch], 2 * d.H, d.H, 0);
                j.add = d.gate_inputs[ch] ? d.gate_inputs[ch] + t * 2 * BH : nullptr; j.ld_add = 2 * d.H;
            }
            PL_TRY(launch_jobs(jobs, d.nchain, st));
            for (int ch = 0; ch < d.nchain; ++ch) {
                const int t = d.reverse[ch] ? d.T - 1 - s : s;
                SkJob& j = jobs[ch];
                sk_gru_cand_job(j, d.B, d.H, d.h[ch] + s * BH, d.z[ch] + t * BH, d.c[ch] + t * BH, d.h[ch] + (s + 1) * BH);
                j.nseg = 1;
                j.seg[0] = sk_seg(d.rh[ch] + t * BH, d.H, d.Wc[ch], d.H, d.H, 0);
                j.add = d.inputs[ch] ? d.inputs[ch] + t * BH : nullptr; j.ld_add = d.H;
                j.mask = d.mask ? d.mask + (size_t)t * d.B : nullptr;
            }
            PL_TRY(launch_jobs(jobs, d.nchain, st));
        }
        return 0;
    }

    int bwd(hipStream_t st) {
        const size_t BH = (size_t)d.B * d.H;
        for (int s = d.T - 1; s >= 0; --s) {
            GruStateBwdArgs ga;
            ga.nchain = d.nchain; ga.B = d.B; ga.H = d.H;
            SkJob jx[4], jy[4];
            for (int ch = 0; ch < d.nchain; ++ch) {
                const int t = d.reverse[ch] ? d.T - 1 - s : s;
                GruStateBwdChain& c = ga.chain[ch];
                c.dh = d.dh[ch] + (s + 1) * BH;
                c.dh2 = nullptr;
                c.hprev = d.h[ch] + s * BH;
                c.z = d.z[ch] + t * BH;
                c.c = d.c[ch] + t * BH;
                c.mask = d.mask ? d.mask + (size_t)t * d.B : nullptr;
                c.dC = d.dC[ch] + t * BH;
                c.dG = d.dG[ch] + t * 2 * BH;
                c.dhprev = d.dh[ch] + s * BH;

                SkJob& x = jx[ch];
                sk_bwd_rh_job(x, d.B, d.H, d.h[ch] + s * BH, d.r[ch] + t * BH, d.dG[ch] + t * 2 * BH + d.H, 2 * d.H,
                              d.dh[ch] + s * BH);
                x.nseg = 1;
                x.seg[0] = sk_seg(d.dC[ch] + t * BH, d.H, d.Wc[ch], d.H, d.H, 1);

                SkJob& y = jy[ch];
                sk_linear_job(y, sk_seg(d.dG[ch] + t * 2 * BH, 2 * d.H, d.Wg[ch], 2 * d.H, 2 * d.H, 1), d.B, d.H, d.H,
                              d.dh[ch] + s * BH, d.H, 1);
            }
            PL_TRY(gru_state_bwd_launch(ga, st));
            PL_TRY(launch_jobs(jx, d.nchain, st));
            PL_TRY(launch_jobs(jy, d.nchain, st));
        }
        return 0;
    }
};

// ----------------------------------------------------------------------------- LSTM scan
struct LstmSeqPlan : PlanBase {
    ParrotLstmSeqDesc d;
    int enqueue(int which, hipStream_t s) override { return which == 0 ? fwd(s) : bwd(s); }

    int fwd(hipStream_t st) {
        const size_t BH = (size_t)d.B * d.H;
        for (int t = 0; t < d.T; ++t) {
            SkJob j;
            sk_lstm_job(j, d.B, d.H, d.c + t * BH, d.c + (t + 1) * BH, d.gates + (size_t)t * 4 * BH, d.s + (t + 1) * BH);
            j.nseg = 1;
            j.seg[0] = sk_seg(d.s + t * BH, d.H, d.W, 4 * d.H, d.H, 0);
            j.add = d.pre_in + (size_t)t * 4 * BH; j.ld_add = 4 * d.H;
            PL_TRY(launch_jobs(&j, 1, st));
        }
        return 0;
    }

    int bwd(hipStream_t st) {
        const size_t BH = (size_t)d.B * d.H;
        for (int t = d.T - 1; t >= 0; --t) {
            PL_TRY(lstm_state_bwd_launch(d.dS + (t + 1) * BH, nullptr, d.dc, d.gates + (size_t)t * 4 * BH, d.c + t * BH,
                                         d.c + (t + 1) * BH, d.dP + (size_t)t * 4 * BH, d.B, d.H, st));
            SkJob y;
            sk_linear_job(y, sk_seg(d.dP + (size_t)t * 4 * BH, 4 * d.H, d.W, 4 * d.H, 4 * d.H, 1), d.B, d.H, d.H, d.dS + t * BH,
                          d.H, 1);
            PL_TRY(launch_jobs(&y, 1, st));
        }
        return 0;
    }
};

// ----------------------------------------------------------------------------- decoder (training)
// Reads top-down: what a plan is (state, entry points) -> descriptor accessors and segment helpers -> job and chain
// builders -> forward schedules (0, 5, 7, 3) -> backward schedules (0, 8, 3) -> the persistent build -> resolve(), the one
// place that decides which of them a descriptor runs.
struct DecoderPlan : PlanBase {
    ParrotDecoderDesc d;

    // ---- what resolve() decides ---------------------------------------------------------------------------------------
    // Schedules (PARROT_SCHEDULE; 3 needs seq buffers for the upper layers).  cfg2 (T=800, B=64, H=1024, L=2) on MI355X,
    // fwd/bwd ms at the time each was measured against schedule 0:
    //   0 merged wavefront launches, one stream (default)                         46 / 60
    //   1 stream per layer with per-step events in one graph (removed)            69 / 105  (0: 56 / 78)
    //   2 chunked layer pipeline, one graph per (layer, chunk) piece, 2 streams   57 / 94   (0: 56 / 78)   (removed)
    //   3 chunk-skewed merged wavefront with hoisted projections, one stream      49 / 70   (0: 46 / 60)
    //   4 persistent forward scan (opt-in; persist_ok): only matches the launch schedules at cfg2
    //   5 balanced wavefront (GRU stacks, L >= 2): forward scan 29.2 -> 25.2 ms, see fwd5
    //   7 one launch per tick (LSTM layers), see fwd7
    // The per-step kernels are latency-bound: a merged launch costs ~9 us + ~7.7 us per 1024 of its longest K, so
    // moving K from the step kernels to batched GEMMs (2, 3) or splitting layers over streams (1, 2) buys less than
    // the extra kernels / GEMMs cost.  layer_norm needs the hoisted projections (they are the ones that must be
    // normalised); layer_norm with L >= 2 therefore runs on 3.
    int schedule = 0, chunk = 50;
    int esplit = 1;
    int full_wgs = 0;    // (launch_jobs: 0 = the step kernel's own tile heuristic)
    bool tiled = false;  // weight operands: the fragment-major copies the caller gave (else the plain packed matrices)
    // Schedule 5: the rows of w of an upper layer's input projection ride in that layer's own step jobs (see fwd5)
    bool s5_w_in_step = true;
    // Schedule 7: att_flags = [T + 2] arrival counters, one per tick; with bf16 operands the backward tick of LSTM layers is
    // ONE launch too (skinny.hip wkb_kernel; bwd_fused), bwd_flags = [ticks x 4 chains] arrival counters.  Both plan-owned,
    // allocated outside any stream capture, zeroed at the head of their scan.
    unsigned* att_flags = nullptr;
    unsigned* bwd_flags = nullptr;
    bool flags_fake = false;  // (placeholders for CPU-only schedule tracing: never dereferenced, never freed)
    bool bwd_fused = false;
    // LSTM layers, bf16 operands, second accumulators given (ParrotDecoderDesc::dh_b ...): the backward products in two K
    // halves.  A wide workgroup streams its whole [B, 4H] operand: 156 workgroups of ~40 us each at cfg4, whatever
    // their width, and 100 idle CUs; two K halves = 312 workgroups of ~20 us.
    // (Layer 0's products in FOUR K parts measured slower, cfg4 94.6 vs 91.4 ms -- 112 narrow workgroups with a ring fill
    // each cost more than the shorter stream returns -- and are not built.)
    bool bwd_ksplit = false;
    bool bwd_hetero = false;  // the K-balanced backward tick (bwd8)
    bool persist_ok = false;  // schedule 4 took the forward scan (build_persist)
    PmProgram pm_prog;

    ~DecoderPlan() override {
        if (att_flags && !flags_fake) (void)hipFree(att_flags);
        if (bwd_flags && !flags_fake) (void)hipFree(bwd_flags);
    }

    int run(int which, hipStream_t s) override {
        BgPrecisionScope precision(d.bf16 ? 1 : -1);
        return PlanBase::run(which, s);
    }

    int enqueue(int which, hipStream_t s) override {
        BgPrecisionScope precision(d.bf16 ? 1 : -1);  // the hoisted projections follow the plan's operand mode (f32 plans: the process-wide one)
        if (which == 0 && persist_ok) return pm_launch(pm_prog, s);  // schedule 4: the persistent phase machine
        if (schedule == 3) return which == 0 ? fwd_skew(s) : bwd_skew(s);
        if (which == 1 && bwd_hetero && (schedule == 0 || schedule == 5)) return bwd8(s);
        if (schedule == 5) return which == 0 ? fwd5(s) : bwd(s);
        if (schedule == 7) return which == 0 ? fwd7(s) : bwd(s);
        return which == 0 ? fwd(s) : bwd(s);
    }

    // Records what the plan's launches of direction `which` read and write (see Tracer); schedules 0, 5 and 7 only.
    int trace(int which, std::vector<TraceRec>& out, std::vector<TraceJob>* jobs_out = nullptr) {
        if (persist_ok || (schedule != 0 && schedule < 5) || d.layer_norm) return PARROT_ERR_UNSUPPORTED;
        Tracer tr;
        g_tracer = &tr;
        const int rc = enqueue(which, nullptr);
        g_tracer = nullptr;
        out.swap(tr.recs);
        if (jobs_out) jobs_out->swap(tr.jobs);
        return rc;
    }

    // ---- descriptor accessors and segment helpers ---------------------------------------------------------------------
    int krows(int l) const { return d.H + d.E + l * d.H; }
    // Gradient wrt the attention context from layer l's step t: layer 0 multiplies w[t] and owns slot t of its own buffer
    // (dw0 / dw0_b / dw0_c), the upper layers multiply w[t + 1] and share slot t + 1 of theirs (dw / dw_b / dw_c).
    float* dctx(float* of_l0, float* of_upper, int l, int t) const {
        const size_t BE = (size_t)d.B * d.E;
        return l == 0 ? of_l0 + (size_t)t * BE : of_upper + (size_t)(t + 1) * BE;
    }
    // forward product x . W[r0 : r0+K, :] of layer l's matrix g (0: Wg, 1: Wc), width ldw
    SkSeg fseg(const float* A, int lda, int l, int g, int r0, int K, int ldw) const {
        if (tiled) {
            const float* Wt = g == 0 ? d.Wg_f[l] : d.Wc_f[l];
            if (d.bf16) return sk_seg(A, lda, Wt + (size_t)(r0 >> 5) * 256, (krows(l) >> 5) * 256, K, 3);
            return sk_seg(A, lda, Wt + (size_t)(r0 >> 4) * 256, (krows(l) >> 4) * 256, K, 2);
        }
        const float* W = g == 0 ? d.Wg[l] : d.Wc[l];
        return sk_seg(A, lda, W + (size_t)r0 * ldw, ldw, K, 0);
    }
    // backward product dP . W[r0 : r0+N, :]^T (K = ldw = width of the matrix)
    SkSeg rseg(const float* A, int l, int g, int r0, int ldw) const {
        if (tiled) {
            const float* Wt = g == 0 ? d.Wg_r[l] : d.Wc_r[l];
            if (d.bf16) return sk_seg(A, ldw, Wt + (size_t)(r0 >> 4) * (ldw >> 5) * 256, (ldw >> 5) * 256, ldw, 3);
            return sk_seg(A, ldw, Wt + (size_t)(r0 >> 4) * (ldw >> 4) * 256, (ldw >> 4) * 256, ldw, 2);
        }
        const float* W = g == 0 ? d.Wg[l] : d.Wc[l];
        return sk_seg(A, ldw, W + (size_t)r0 * ldw, ldw, ldw, 1);
    }
    // backward product dP[:, k0 : k0 + K] . W[r0 : r0 + N, k0 : k0 + K]^T over the fragment-major reverse copies
    SkSeg rseg_k(const float* A, int l, int g, int r0, int ldw, int k0, int K) const {
        const float* Wt = g == 0 ? d.Wg_r[l] : d.Wc_r[l];
        return sk_seg(A + k0, ldw, Wt + ((size_t)(r0 >> 4) * (ldw >> 4) + (k0 >> 4)) * 256, (ldw >> 4) * 256, K, 2);
    }

    // Adds the K-segments [h_l ; w ; h_0..h_{l-1}] against layer l's matrix g (row-major [K_l, ldw]).
    void layer_segs(SkJob& j, int l, int t, const float* first, int g, int ldw) const {
        const size_t BH = (size_t)d.B * d.H, BE = (size_t)d.B * d.E;
        int n = 0;
        j.seg[n++] = fseg(first, d.H, l, g, 0, d.H, ldw);
        const float* wsrc = d.w + (size_t)(l == 0 ? t : t + 1) * BE;
        j.seg[n++] = fseg(wsrc, d.E, l, g, d.H, d.E, ldw);
        for (int q = 0; q < l; ++q)
            j.seg[n++] = fseg(d.h[q] + (size_t)(t + 1) * BH, d.H, l, g, d.H + d.E + q * d.H, d.H, ldw);
        j.nseg = n;
    }
    // The layer's own recurrent block (+ w_{t-1} for layer 0): what a step job of schedule 3 keeps.
    void own_segs(SkJob& j, int l, int t, const float* first, int g, int ldw) const {
        const size_t BE = (size_t)d.B * d.E;
        j.seg[0] = fseg(first, d.H, l, g, 0, d.H, ldw);
        j.nseg = 1;
        if (l == 0) j.seg[j.nseg++] = fseg(d.w + (size_t)t * BE, d.E, l, g, d.H, d.E, ldw);
    }

    // The additive-input buffer of layer l is live when the caller filled it (seq_init bit) or when the
    // pipeline schedule batches the lower layers' projections into it.
    bool has_seq(int l, const float* p) const { return p && (((d.seq_init >> l) & 1) || (schedule >= 2 && schedule != 7 && l > 0)); }

    // ---- job and chain builders ---------------------------------------------------------------------------------------
    void gates_job(SkJob& j, int l, int t) const {
        const size_t BH = (size_t)d.B * d.H;
        sk_gru_gates_job(j, d.B, d.H, d.h[l] + t * BH, d.z[l] + t * BH, d.r[l] + t * BH, d.rh[l] + t * BH);
        layer_segs(j, l, t, d.h[l] + t * BH, 0, 2 * d.H);
        j.bias = d.bg[l];
        j.add = has_seq(l, d.seq_g[l]) ? d.seq_g[l] + t * 2 * BH : nullptr; j.ld_add = 2 * d.H;
    }

    void cand_job(SkJob& j, int l, int t) const {
        const size_t BH = (size_t)d.B * d.H;
        sk_gru_cand_job(j, d.B, d.H, d.h[l] + t * BH, d.z[l] + t * BH, d.c[l] + t * BH, d.h[l] + (t + 1) * BH);
        layer_segs(j, l, t, d.rh[l] + t * BH, 1, d.H);
        j.bias = d.bc[l];
        j.add = has_seq(l, d.seq_c[l]) ? d.seq_c[l] + t * BH : nullptr; j.ld_add = d.H;
    }

    void lstm_job(SkJob& j, int l, int t) const {
        const size_t BH = (size_t)d.B * d.H;
        sk_lstm_job(j, d.B, d.H, d.cst[l] + t * BH, d.cst[l] + (t + 1) * BH, d.gate4[l] + t * 4 * BH, d.h[l] + (t + 1) * BH);
        layer_segs(j, l, t, d.h[l] + t * BH, 0, 4 * d.H);
        j.bias = d.bg[l];
        j.add = has_seq(l, d.seq_g[l]) ? d.seq_g[l] + t * 4 * BH : nullptr; j.ld_add = 4 * d.H;
    }

    // Input projection of layer l >= 1 for step t (schedule 5): [w_{t+1} ; h_0 .. h_{l-1}] . W[H:, :] into the layer's
    // additive-input buffer.  part 0: the whole projection; 1: the rows of w and h_0 .. h_{l-2} (ready a tick earlier);
    // 2: the rows of h_{l-1}, accumulated onto part 1 (two jobs of about the recurrent K instead of one of K = E + l H).
    // no_w: the rows of w are not in this job (they ride in the layer's own step job, s5_w_in_step).
    void input_job(SkJob& j, int l, int t, int g, int part = 0, bool no_w = false) const {
        const size_t BH = (size_t)d.B * d.H, BE = (size_t)d.B * d.E;
        const int wd = d.cell == 1 ? 4 * d.H : (g == 0 ? 2 * d.H : d.H);  // LSTM layers: one 4H-wide matrix (g = 0)
        // (accumulate: part 2 onto part 1; otherwise onto caller data -- feedback / speaker terms -- already there)
        sk_linear_job(j, d.B, wd, d.H, (g == 0 ? d.seq_g[l] : d.seq_c[l]) + (size_t)t * d.B * wd, wd,
                      part == 2 ? 1 : ((d.seq_init >> l) & 1));
        j.colmode = d.cell == 1 && tiled ? 1 : 0;  // (the tiled copies of LSTM matrices keep the gate-interleaved tile order)
        int n = 0;
        if (part != 2 && !no_w) j.seg[n++] = fseg(d.w + (size_t)(t + 1) * BE, d.E, l, g, d.H, d.E, wd);
        for (int q = 0; q < l; ++q) {
            if ((part == 1 && q == l - 1) || (part == 2 && q != l - 1)) continue;
            j.seg[n++] = fseg(d.h[q] + (size_t)(t + 1) * BH, d.H, l, g, d.H + d.E + q * d.H, d.H, wd);
        }
        j.nseg = n;
    }

    AttFwdArgs att_fwd_args(int t) const {
        const size_t BH = (size_t)d.B * d.H, BE = (size_t)d.B * d.E, BA = (size_t)d.B * d.A;
        AttFwdArgs g{};
        g.h1 = d.h[0] + (t + 1) * BH; g.ldh = d.H;
        g.WattT = d.WattT; g.batt = d.batt;
        g.kappa_prev = d.kappa + t * BA;
        g.ctx = d.ctx;
        g.a_out = d.a + t * BA; g.b_out = d.b + t * BA; g.kappa_out = d.kappa + (t + 1) * BA;
        g.phi_out = d.phi + (size_t)t * d.B * d.U;
        g.w_out = d.w + (t + 1) * BE; g.ldw = d.E;
        g.B = d.B; g.H = d.H; g.A = d.A; g.U = d.U; g.E = d.E; g.esplit = esplit;
        g.att_type = d.att_type; g.eps = d.eps; g.alignment = d.alignment;
        g.sharpening = d.sharpening; g.timing = d.timing;
        g.sup_out = d.att_sup ? d.att_sup + (size_t)t * d.B * 2 : nullptr;
        return g;
    }
    int att_fwd_step(int t, hipStream_t st) const { return traced_att_fwd_launch(att_fwd_args(t), st); }

    // Arguments of the attention backward of step t0 (one place: every backward schedule uses it).
    AttBwdArgs att_bwd_args(int t0) const {
        const size_t BH = (size_t)d.B * d.H, BE = (size_t)d.B * d.E, BA = (size_t)d.B * d.A;
        AttBwdArgs g{};
        g.dw = d.dw + (t0 + 1) * BE; g.dw2 = d.dw0 + (t0 + 1) * BE; g.lddw = d.E;
        g.ctx = d.ctx;
        g.a = d.a + t0 * BA; g.b = d.b + t0 * BA;
        g.kappa = d.kappa + (t0 + 1) * BA; g.kappa_prev = d.kappa + t0 * BA;
        g.WattT = d.WattT;
        g.dkappa = d.dkappa;
        g.dp_out = d.dp + (size_t)t0 * d.B * 3 * d.A;
        g.sup = d.att_sup ? d.att_sup + (size_t)t0 * d.B * 2 : nullptr;
        g.dh1 = d.dh[0] + (t0 + 1) * BH; g.lddh = d.H;
        g.B = d.B; g.H = d.H; g.A = d.A; g.U = d.U; g.E = d.E; g.att_type = d.att_type; g.eps = d.eps;
        return g;
    }

    // State backward of layer l at step t: reads dh[t + 1] (+ the share the layers above left in dhup), leaves dC / dG_z
    // (GRU) or dP (LSTM) and adds into dh[t].  The K-split ticks add their further shares (dhx / dh3, dh4) afterwards.
    GruStateBwdChain gru_chain(int l, int t) const {
        const size_t BH = (size_t)d.B * d.H;
        GruStateBwdChain c;
        c.dh = d.dh[l] + (t + 1) * BH;
        c.dh2 = (l + 1 < d.L) ? d.dhup[l] + (t + 1) * BH : nullptr;
        c.hprev = d.h[l] + t * BH;
        c.z = d.z[l] + t * BH;
        c.c = d.c[l] + t * BH;
        c.mask = nullptr;
        c.dC = d.dC[l] + t * BH;
        c.dG = d.dG[l] + t * 2 * BH;
        c.dhprev = d.dh[l] + t * BH;
        return c;
    }
    LstmStateBwdChain lstm_chain(int l, int t) const {
        const size_t BH = (size_t)d.B * d.H;
        LstmStateBwdChain c;
        c.dh = d.dh[l] + (t + 1) * BH;
        c.dh2 = (l + 1 < d.L) ? d.dhup[l] + (t + 1) * BH : nullptr;
        c.dc = d.dcell[l];
        c.gates = d.gate4[l] + (size_t)t * 4 * BH;
        c.c_prev = d.cst[l] + t * BH;
        c.c_new = d.cst[l] + (t + 1) * BH;
        c.dP = d.dG[l] + (size_t)t * 4 * BH;
        return c;
    }

    // d(r*h_prev) = dC . Wc[0:H, :]^T of layer l at step t; epilogue -> dG_r, dh_prev += d(rh) * r
    void rh_job(SkJob& x, int l, int t) const {
        const size_t BH = (size_t)d.B * d.H;
        const int H = d.H;
        sk_bwd_rh_job(x, d.B, H, d.h[l] + t * BH, d.r[l] + t * BH, d.dG[l] + t * 2 * BH + H, 2 * H, d.dh[l] + t * BH);
        x.nseg = 1;
        x.seg[0] = rseg(d.dC[l] + t * BH, l, 1, 0, H);
    }
    // The transposed products into gradient buffers, out (+)= sg.A . sg.B^T, are single-segment sk_linear_job()s.
    // ... in two K halves (bwd_ksplit): the second half's sums go to `second`, stored, or added when several jobs of a
    // window share the destination (`added`; such a buffer is caller-zeroed).  Not an epilogue's wiring: a split LINEAR job
    // reuses o1 / ldo1 for the second half's destination and ldo2 as the `added` flag (skinny.h, ksplit), so it stays here.
    static void ksplit2(SkJob& j, float* second, int ld, int added) {
        j.ksplit = 2;
        j.o1 = second; j.ldo1 = ld;
        j.ldo2 = added;
    }

    // ---- schedule 0, forward: the merged wavefront ---------------------------------------------------------------------
    // At tick q layer l advances step t = q - l, so the gate GEMMs of all layers share
    // one launch, the candidate GEMMs a second one, and the attention of step q is the third.  Layer
    // l >= 1 needs h_j(t) (j < l) and w_t, both produced in earlier ticks; layer 0 needs w_{t-1}.
    int nticks() const { return d.T + d.L - 1; }
    int fwd(hipStream_t st) {
        for (int q = 0; q < nticks(); ++q) {
            SkJob jobs[PARROT_MAX_LAYERS];
            int n = 0;
            if (d.cell == 1) {  // LSTM layers: a single fused GEMM + cell update per layer-step
                for (int l = 0; l < d.L; ++l) {
                    const int t = q - l;
                    if (t >= 0 && t < d.T) lstm_job(jobs[n++], l, t);
                }
                PL_TRY(launch_jobs(jobs, n, st, full_wgs));
                if (q < d.T) PL_TRY(att_fwd_step(q, st));
                continue;
            }
            for (int l = 0; l < d.L; ++l) {
                const int t = q - l;
                if (t >= 0 && t < d.T) gates_job(jobs[n++], l, t);
            }
            PL_TRY(launch_jobs(jobs, n, st, full_wgs));
            n = 0;
            for (int l = 0; l < d.L; ++l) {
                const int t = q - l;
                if (t >= 0 && t < d.T) cand_job(jobs[n++], l, t);
            }
            PL_TRY(launch_jobs(jobs, n, st, full_wgs));
            if (q < d.T) PL_TRY(att_fwd_step(q, st));
        }
        return 0;
    }

    // ---- schedule 5: balanced wavefront (GRU layers, L >= 2) --------------------------------------------------------
    // A step launch costs ~4.7 us + ~4.8 us per 1024 of the LONGEST K among its workgroups (tools/skbench4.hip,
    // profiles/r03_launch_cost_model.txt): in schedule 0 the upper layers' workgroups (K = 2H + E and more) set the
    // pace of both GEMM launches while layer 0's finish early, and the attention launch leaves the chip idle.  Here
    // the products of layer l >= 1 are cut in two: the INPUT projection [w_t ; h_0 .. h_{l-1}] . W[H:, :] (everything
    // that comes from below, ready one tick before it is needed) is a separate linear job that writes the layer's
    // additive-input buffer seq_g / seq_c and rides in the launch of the ATTENTION step (heterogeneous launch,
    // skinny.hip ska_kernel); the gate / candidate launches keep only the recurrent K = H of the upper layers next to
    // layer 0's K = H + E.  Layer l >= 1 lags l + 1 ticks.  Per tick q:
    //   A: gates(l0, q), gates_rec(l, q - l - 1)     B: cand(l0, q), cand_rec(l, q - l - 1)
    //   C: attention(q) + input projections of layer l for step q - l (all l >= 1)
    // The pre-activation of an upper layer is now (recurrent sum) + (input sum) instead of one running sum over the
    // concatenated K: same terms, other rounding (not bit-identical to schedule 0; the oracle tests cover both).
    //
    // GRU layers l >= 2 (the reference's own depth: model.py:312-347), `gsplit`: the input projection walks K = E + l H
    // (2304 at l = 2) -- the longest K of its launch by far, in a launch that already holds 1.75 rounds of workgroups
    // (25.8 us at three layers).  It is cut like the LSTM one: part 1 = the rows of w and h_0 .. h_{l-2}, ready two ticks
    // before the rows of h_{l-1}, rides in the gate launch (the gate block) and the candidate launch (the candidate block) of
    // the tick in between -- both are 1.5 rounds there and take the extra half round for nothing --, part 2 = the rows of
    // h_{l-1} stays in the attention launch and accumulates.  No job of a tick walks more than K = H + E.
    //
    // s5_w_in_step (PARROT_S5_WSTEP=0 opts out): the rows of w of an upper layer's input projection (K = E) ride in that
    // layer's OWN gate / candidate job (a second segment behind the recurrent block: w_{t+1} is two ticks old by then)
    // instead of the attention launch's projection jobs.  At two layers the gate launch holds K = H + E (layer 0) beside
    // K = H (layer 1) workgroups, one per CU, and the candidate launch likewise: the upper layers' workgroups walk the
    // extra E rows while layer 0's are still busy, and the attention launch -- bound by its GEMM workgroups since the
    // attention chain shrank -- walks K = l H instead of E + l H.
    int lag5(int l) const { return l == 0 ? 0 : l + 1; }
    int nticks5() const { return d.T + lag5(d.L - 1); }
    int fwd5(hipStream_t st) {
        const int Q = nticks5();
        const int cfull = 160;  // workgroup count at which the heterogeneous launch keeps 32 x 32 tiles (measured)
        // launches of a tick: <= L gate jobs (+ part 1 of the upper layers' gate projections), <= L candidate jobs (+ part 1
        // of the candidate projections), <= 3 input-projection jobs per upper layer
        static_assert(3 * (PARROT_MAX_LAYERS - 1) <= SK_MAXJOB && 2 * PARROT_MAX_LAYERS - 2 <= SK_MAXJOB, "fwd5: jobs[] too short");
        const bool gsplit = d.cell == 0 && d.L >= 3;
        const bool wstep = s5_w_in_step;
        for (int q = 0; q < Q; ++q) {
            SkJob jobs[SK_MAXJOB];
            int n = 0;
            for (int l = 0; l < d.L; ++l) {
                const int t = q - lag5(l);
                if (t < 0 || t >= d.T) continue;
                SkJob& j = jobs[n++];
                if (d.cell == 1) lstm_job(j, l, t);  // LSTM layers: one fused product + cell update per layer-step
                else gates_job(j, l, t);
                if (l > 0) j.nseg = wstep ? 2 : 1;  // recurrent block (+ the rows of w); the rest arrives through seq_g (has_seq)
            }
            if (gsplit)
                for (int l = 2; l < d.L; ++l) {  // part 1 of the step whose part 2 the attention launch of THIS tick adds
                    const int tp = q - lag5(l) + 1;
                    if (tp >= 0 && tp < d.T) input_job(jobs[n++], l, tp, 0, 1, wstep);
                }
            if (n > 0) PL_TRY(launch_jobs(jobs, n, st, full_wgs));
            n = 0;
            if (d.cell == 0) {
                for (int l = 0; l < d.L; ++l) {
                    const int t = q - lag5(l);
                    if (t < 0 || t >= d.T) continue;
                    SkJob& j = jobs[n++];
                    cand_job(j, l, t);
                    if (l > 0) j.nseg = wstep ? 2 : 1;
                }
                if (gsplit)
                    for (int l = 2; l < d.L; ++l) {
                        const int tp = q - lag5(l) + 1;
                        if (tp >= 0 && tp < d.T) input_job(jobs[n++], l, tp, 1, 1, wstep);
                    }
                if (n > 0) PL_TRY(launch_jobs(jobs, n, st, full_wgs));
            }
            n = 0;
            for (int l = 1; l < d.L; ++l) {
                const int t = q - lag5(l) + 1;
                // LSTM input projections of l >= 2 as two K-balanced jobs (one job measured slower)
                const bool split = d.cell == 1 && l >= 2;
                const bool gs = gsplit && l >= 2;  // (part 1 was written by the gate / candidate launches of this tick)
                if (t >= 0 && t < d.T) {
                    input_job(jobs[n++], l, t, 0, (split || gs) ? 2 : 0, wstep);
                    if (d.cell == 0) input_job(jobs[n++], l, t, 1, gs ? 2 : 0, wstep);
                }
                if (split) {  // the rows that were ready a tick earlier
                    const int ta = t + 1;
                    if (ta >= 0 && ta < d.T) input_job(jobs[n++], l, ta, 0, 1, wstep);
                }
            }
            if (q < d.T) {
                AttFwdArgs ag = att_fwd_args(q);
                if (n > 0) ag.esplit = 1;  // beside GEMM workgroups: one attention workgroup per batch row (measured)
                PL_TRY(launch_jobs_att(jobs, n, ag, st, cfull));
            } else if (n > 0) PL_TRY(launch_jobs(jobs, n, st, full_wgs));
        }
        return 0;
    }

    // ---- schedule 7: ONE launch per tick for LSTM layers -------------------------------------------------------------
    // Schedule 0 runs an LSTM tick as the fused launch of all layers (wk_kernel at cfg4: ~35 us, bound by its total work)
    // followed by the attention step ALONE (~12.6 us: a chain of dependent round trips on 64 CUs, the other 192 idle).
    // The attention of step q-1 only feeds the LAST K = E rows of layer 0's product at step q (and the upper layers a
    // tick later), and an LSTM launch is three times as long as the attention chain.  So the attention rides at the head
    // of the next tick's launch: its blocks are dispatched first and publish w write-through plus an arrival count
    // (att_fwd_body.h); layer 0's workgroups -- the shortest K of the launch -- come LAST in the grid,
    // start on the CUs the attention blocks free, walk their h rows and take the w rows behind the flag (wk_body's tail;
    // sk_body's for f32 operands).  The upper layers lag one tick more than in schedule 0 so that the w they read was
    // published by an EARLIER launch:  tick q:  attention(q-1) || lstm(l0, q) [w rows flagged], lstm(l, q - lag7(l)),
    // lag7 = 0, 2, 3.  Same terms per output element as schedule 0 (the attention runs one block per batch row here, so
    // its sums differ from schedule 0's column-sliced blocks in the last bits).
    int lag7(int l) const { return l == 0 ? 0 : l + 1; }
    int nticks7() const { return d.T + std::max(1, lag7(d.L - 1)); }
    int fwd7(hipStream_t st) {
        if (!att_flags) return PARROT_ERR_BADARG;  // (allocated by resolve(), outside any stream capture)
        if (!g_tracer) PL_TRY(sk_zero_words_launch(att_flags, d.T + 2, st));
        const int Q = nticks7();
        for (int q = 0; q < Q; ++q) {
            SkJob jobs[PARROT_MAX_LAYERS];
            int n = 0;
            const bool att_on = q >= 1 && q - 1 < d.T;
            AttFwdArgs ag{};
            if (att_on) {
                ag = att_fwd_args(q - 1);
                ag.esplit = 1;  // beside GEMM workgroups: one attention workgroup per batch row
            }
            for (int l = 0; l < d.L; ++l) {
                const int t = q - lag7(l);
                if (t < 0 || t >= d.T) continue;
                SkJob& j = jobs[n++];
                lstm_job(j, l, t);
                if (l == 0 && att_on) {  // w_{q-1} arrives inside this launch: its segment goes last and waits
                    if (j.nseg != 2) return PARROT_ERR_BADARG;
                    j.wait_flag = att_flags + q;
                    j.wait_target = (unsigned)(ag.B * ag.esplit);
                    ag.flag = att_flags + q;
                }
            }
            if (att_on) PL_TRY(launch_jobs_att(jobs, n, ag, st, 0));
            else if (n > 0) PL_TRY(launch_jobs(jobs, n, st, full_wgs));
        }
        return 0;
    }

    // ---- schedule 3: skewed wavefront with hoisting -------------------------------------------------
    // Merged launches as in schedule 0, but layer l lags layer l-1 by one CHUNK of steps instead of one step.
    // Layer l >= 1 only consumes finished outputs of the layers below (h_j(t), w_t), never the other way round (this is the
    // "chunked layer pipeline" the seq buffers of ParrotDecoderDesc were added for).  When layer l-1 has finished a chunk,
    // the Fork projections of its outputs (and of w) into layer l (the Fork bricks h{j}_to_h{l} / inp_to_h{l},
    // model.py:692-722) are taken for the whole chunk by the LDS-tiled GEMM (hoist_fwd: M = chunk*B rows instead of B)
    // into the layer's additive-input buffer seq_g / seq_c, so every per-step job keeps only the layer's own
    // recurrent block (+ w_{t-1} for layer 0): the slowest workgroups of a merged launch shrink from
    // K = H+E+lH to K <= H+E, and ~36 % of the step-kernel flops move to a kernel that runs at 115+ TFLOP/s.
    // One stream, one graph; costs (L-1) extra chunks of (light) ticks at the ends.

    // Group g (0: the gates, or an LSTM layer's one 4H-wide matrix; 1: the candidate) of layer l's hoisted projections:
    // its matrix [krows(l), wd] and the row blocks that multiply w and h_j.
    struct HoistGroup {
        int wd, H, E;
        const float* W;
        const float* w_rows() const { return W + (size_t)H * wd; }
        const float* h_rows(int j) const { return W + (size_t)(H + E + j * H) * wd; }
    };
    int hoist_groups() const { return d.cell == 1 ? 1 : 2; }
    HoistGroup hoist_group(int l, int g) const {
        return {d.cell == 1 ? 4 * d.H : (g == 0 ? 2 * d.H : d.H), d.H, d.E, g == 0 ? d.Wg[l] : d.Wc[l]};
    }
    // layer_norm: what the (l, j) pair of group g keeps for steps t0.. -- the normalised projection (the backward leaves the
    // pre-norm gradient there), the row std, and the Fork's own bias
    struct LnBufs { float* y; float* sigma; const float* bias; };
    LnBufs ln_bufs(int l, int j, int g, int t0, int wd) const {
        const int pj = l * PARROT_MAX_LAYERS + j;
        return {(g == 0 ? d.ln_yg[pj] : d.ln_yc[pj]) + (size_t)t0 * d.B * wd,
                (g == 0 ? d.ln_sg[pj] : d.ln_sc[pj]) + (size_t)t0 * d.B, g == 0 ? d.ln_bg[pj] : d.ln_bc[pj]};
    }

    int hoist_fwd(int l, int t0, int t1, hipStream_t st) const {
        const int H = d.H, E = d.E, R = (t1 - t0) * d.B;
        const size_t BH = (size_t)d.B * H, BE = (size_t)d.B * E;
        for (int g = 0; g < hoist_groups(); ++g) {
            const HoistGroup hg = hoist_group(l, g);
            const int wd = hg.wd;
            float* out = (g == 0 ? d.seq_g[l] : d.seq_c[l]) + (size_t)t0 * d.B * wd;
            int acc = (d.seq_init >> l) & 1;
            PL_TRY(parrot_gemm(d.w + (size_t)(t0 + 1) * BE, E, 0, hg.w_rows(), wd, 0, out, wd, R, wd, E,
                               nullptr, 1.f, acc, 0, 1, 0, 0, 0, 1, st));
            for (int j = 0; j < l; ++j) {
                const float* A = d.h[j] + (size_t)(t0 + 1) * BH;
                const float* Wj = hg.h_rows(j);
                if (!d.layer_norm) {
                    PL_TRY(parrot_gemm(A, H, 0, Wj, wd, 0, out, wd, R, wd, H, nullptr, 1.f, 1, 0, 1, 0, 0, 0, 1, st));
                    continue;
                }
                // layer_norm: project (with the Fork's own bias), normalise each row, then add (model.py:703-722)
                const LnBufs ln = ln_bufs(l, j, g, t0, wd);
                PL_TRY(parrot_gemm(A, H, 0, Wj, wd, 0, ln.y, wd, R, wd, H, ln.bias, 1.f, 0, 0,
                                   1, 0, 0, 0, 1, st));
                PL_TRY(simple_norm_fwd_launch(ln.y, wd, ln.y, wd, ln.sigma, R, wd, PARROT_NORM_EPS, out, wd, st));
            }
        }
        return 0;
    }

    // Gradients of the hoisted projections for one chunk: dw[t+1] and dhup[p][t+1] += dPre . W^T.
    int hoist_bwd(int l, int t0, int t1, hipStream_t st) const {
        const int H = d.H, E = d.E, R = (t1 - t0) * d.B;
        const size_t BH = (size_t)d.B * H, BE = (size_t)d.B * E;
        for (int g = 0; g < hoist_groups(); ++g) {
            const HoistGroup hg = hoist_group(l, g);
            const int wd = hg.wd;
            const float* dP = (g == 0 ? d.dG[l] : d.dC[l]) + (size_t)t0 * d.B * wd;
            PL_TRY(parrot_gemm(dP, wd, 0, hg.w_rows(), wd, 1, d.dw + (size_t)(t0 + 1) * BE, E, R, E, wd,
                               nullptr, 1.f, 1, 0, 1, 0, 0, 0, 1, st));
            for (int p = 0; p < l; ++p) {
                const float* dsrc = dP;
                if (d.layer_norm) {  // back through the row normalisation; the pre-norm gradient replaces y
                    const LnBufs ln = ln_bufs(l, p, g, t0, wd);
                    PL_TRY(simple_norm_bwd_launch(dP, wd, ln.y, wd, ln.sigma, ln.y, wd, R, wd, PARROT_NORM_EPS, 0, st));
                    dsrc = ln.y;
                }
                PL_TRY(parrot_gemm(dsrc, wd, 0, hg.h_rows(p), wd, 1,
                                   d.dhup[p] + (size_t)(t0 + 1) * BH, H, R, H, wd, nullptr, 1.f, 1, 0, 1, 0, 0, 0, 1,
                                   st));
            }
        }
        return 0;
    }

    int fwd_skew(hipStream_t st) {
        const size_t BH = (size_t)d.B * d.H;
        const int C = ceil_div(d.T, chunk);
        for (int sc = 0; sc < C + d.L - 1; ++sc) {
            for (int l = 1; l < d.L; ++l) {
                const int c = sc - l;
                if (c >= 0 && c < C) PL_TRY(hoist_fwd(l, c * chunk, (c + 1) * chunk < d.T ? (c + 1) * chunk : d.T, st));
            }
            for (int s = 0; s < chunk; ++s) {
                SkJob jobs[PARROT_MAX_LAYERS];
                int n = 0, t0 = -1;
                for (int l = 0; l < d.L; ++l) {
                    const int c = sc - l, t = c * chunk + s;
                    if (c < 0 || c >= C || t >= d.T) continue;
                    if (l == 0) t0 = t;
                    if (d.cell == 1) {
                        lstm_job(jobs[n], l, t);
                        own_segs(jobs[n], l, t, d.h[l] + t * BH, 0, 4 * d.H);
                    } else {
                        gates_job(jobs[n], l, t);
                        own_segs(jobs[n], l, t, d.h[l] + t * BH, 0, 2 * d.H);
                    }
                    ++n;
                }
                if (n == 0) continue;
                PL_TRY(launch_jobs(jobs, n, st));
                if (d.cell == 0) {
                    n = 0;
                    for (int l = 0; l < d.L; ++l) {
                        const int c = sc - l, t = c * chunk + s;
                        if (c < 0 || c >= C || t >= d.T) continue;
                        cand_job(jobs[n], l, t);
                        own_segs(jobs[n], l, t, d.rh[l] + t * BH, 1, d.H);
                        ++n;
                    }
                    PL_TRY(launch_jobs(jobs, n, st));
                }
                if (t0 >= 0) PL_TRY(att_fwd_step(t0, st));
            }
        }
        return 0;
    }

    // ---- schedule 0, backward: the merged wavefront --------------------------------------------------------------------
    // At tick q layer l (upper layers first) handles step t = T-1-(q-(L-1-l)).
    // Per tick: attention backward of layer 0's step, then one elementwise launch, one launch of the
    // d(r*h) GEMMs and one launch of the input-gradient GEMMs for all active layers.
    // Gradient contributions that cross layers land in separate buffers (dhup[l] for the state, dw0
    // for layer 0's share of dw), so no two jobs of a launch update the same element: no atomics, and
    // the result is deterministic.  The consumers add the parts when they read.
    // LSTM layers: with bwd_fused the whole tick is one launch, with bwd_ksplit every product runs in two K halves.
    int bwd(hipStream_t st) {
        const size_t BH = (size_t)d.B * d.H, BE = (size_t)d.B * d.E;
        const int H = d.H, E = d.E;
        if (bwd_fused && !g_tracer) PL_TRY(sk_zero_words_launch(bwd_flags, 4 * nticks(), st));
        for (int q = 0; q < nticks(); ++q) {
            int tl[PARROT_MAX_LAYERS];
            for (int l = 0; l < d.L; ++l) tl[l] = d.T - 1 - (q - (d.L - 1 - l));
            const int t0 = tl[0];
            const bool att_on = t0 >= 0 && t0 < d.T;
            AttBwdArgs g{};
            if (att_on) g = att_bwd_args(t0);
            if (att_on && bwd_ksplit) {  // (LSTM layers) the second K halves' shares of dw
                g.dw3 = d.dw_b + (size_t)(t0 + 1) * BE;
                g.dw4 = d.dw0_b + (size_t)(t0 + 1) * BE;
            }
            if (d.cell == 1) {
                SkJob jl[SK_MAXJOB];
                int nl = 0;
                LstmStateBwdArgs la;
                la.nchain = 0; la.B = d.B; la.H = H;
                int chain_of[PARROT_MAX_LAYERS];
                for (int l = d.L - 1; l >= 0; --l) {  // state updates of all active layers + attention
                    chain_of[l] = -1;
                    const int t = tl[l];
                    if (t < 0 || t >= d.T) continue;
                    chain_of[l] = la.nchain;
                    LstmStateBwdChain& c = la.chain[la.nchain++];
                    c = lstm_chain(l, t);
                    c.dh3 = bwd_ksplit ? d.dh_b[l] + (t + 1) * BH : nullptr;  // the second K halves' sums (below)
                    c.dh4 = (bwd_ksplit && l + 1 < d.L) ? d.dhup_b[l] + (t + 1) * BH : nullptr;
                    c.dP16 = (bwd_fused && d.dG16[l]) ? static_cast<char*>(d.dG16[l]) + (size_t)t * 4 * BH * 2 : nullptr;
                }
                for (int l = d.L - 1; l >= 0; --l) {
                    const int t = tl[l];
                    if (t < 0 || t >= d.T) continue;
                    float* dP = d.dG[l] + (size_t)t * 4 * BH;
                    const int first = nl;
                    SkJob& jh = jl[nl++];  // previous state of this layer
                    sk_linear_job(jh, rseg(dP, l, 0, 0, 4 * H), d.B, H, H, d.dh[l] + t * BH, H, 1);
                    if (bwd_ksplit) ksplit2(jh, d.dh_b[l] + t * BH, H, 0);
                    SkJob& jw = jl[nl++];  // attention context
                    sk_linear_job(jw, rseg(dP, l, 0, H, 4 * H), d.B, E, H, dctx(d.dw0, d.dw, l, t), E, 1);
                    // dw_b[t + 1] collects every upper layer's share: added (caller-zeroed)
                    if (bwd_ksplit) ksplit2(jw, dctx(d.dw0_b, d.dw_b, l, t), E, l == 0 ? 0 : 1);
                    for (int p = 0; p < l; ++p) {  // lower layers' states of the same step
                        SkJob& j = jl[nl++];
                        sk_linear_job(j, rseg(dP, l, 0, H + E + p * H, 4 * H), d.B, H, H, d.dhup[p] + (t + 1) * BH, H, 1);
                        if (bwd_ksplit) ksplit2(j, d.dhup_b[p] + (t + 1) * BH, H, 1);  // (added: all layers above p)
                    }
                    if (bwd_fused)  // the products of a layer read what its chain's rows publish inside the launch
                        for (int q2 = first; q2 < nl; ++q2) {
                            jl[q2].wait_flag = bwd_flags + (size_t)q * 4 + chain_of[l];
                            jl[q2].wait_target = (unsigned)d.B;
                            jl[q2].wait_all = (l == 0 && att_on) ? 2 : 1;  // (2: behind the attention rows, last in the grid)
                        }
                }
                const int l0c = att_on ? la.nchain - 1 : -1;
                if (bwd_fused && la.nchain > 0 && nl > 0) {
                    unsigned* fl[4] = {nullptr, nullptr, nullptr, nullptr};
                    for (int c2 = 0; c2 < la.nchain; ++c2) fl[c2] = bwd_flags + (size_t)q * 4 + c2;
                    const int rc = traced_bwd_fused_launch(att_on ? &g : nullptr, la, l0c, jl, nl, fl, st);
                    if (rc != PARROT_ERR_UNSUPPORTED) {
                        PL_TRY(rc);
                        continue;
                    }
                    for (int q2 = 0; q2 < nl; ++q2) { jl[q2].wait_flag = nullptr; jl[q2].wait_target = 0; jl[q2].wait_all = 0; }
                }
                if (la.nchain > 0) PL_TRY(traced_att_state_bwd_launch(att_on ? &g : nullptr, la, l0c, st));
                // Only the fused tick's row blocks write the bf16 copies of the pre-activation gradients (dG16): on this
                // fall-back path they are made here, so that parrot_decoder_writes_bf16_grads() stays true for every tick
                // (the weight-gradient products would otherwise read rows nobody wrote).
                for (int c2 = 0; c2 < la.nchain; ++c2)
                    if (la.chain[c2].dP16)
                        PL_TRY(bg_to_bf16_launch(la.chain[c2].dP, la.chain[c2].dP16, (long long)d.B * 4 * H, st));
                if (nl > 0) PL_TRY(launch_jobs(jl, nl, st, full_wgs, 0, bwd_ksplit ? 1 : 0));
                continue;
            }
            GruStateBwdArgs ga;
            ga.nchain = 0; ga.B = d.B; ga.H = H;
            // the split backward tick carries 1 + 1 + l jobs per layer in each of the X and Y launches
            static_assert(PARROT_MAX_LAYERS * (PARROT_MAX_LAYERS + 3) / 2 <= SK_MAXJOB,
                          "backward tick: jx / jy cannot hold every layer's jobs");
            SkJob jx[SK_MAXJOB], jy[SK_MAXJOB];
            int nx = 0, ny = 0;
            for (int l = d.L - 1; l >= 0; --l) {
                const int t = tl[l];
                if (t < 0 || t >= d.T) continue;
                ga.chain[ga.nchain++] = gru_chain(l, t);
                // X: d(r*h_prev) and the products with dC (K = H); Y: the products with dG (K = 2H), which need X's dG_r.
                // One job per destination.  The dC products do not need dG_r, so they ride in X and no workgroup of a tick
                // walks K = 3H (a launch costs ~4.7 us + ~4.8 us per 1024 of its LONGEST K: with them in Y
                // 12.0 + 7.9 + 19.9 us per tick, here 12.0 + 9.5 + 14.3 us).
                rh_job(jx[nx++], l, t);
                const float* dG = d.dG[l] + t * 2 * BH;
                const float* dC = d.dC[l] + t * BH;
                // previous state of this layer: only the gate GEMM (rh part handled by X's epilogue)
                sk_linear_job(jy[ny++], rseg(dG, l, 0, 0, 2 * H), d.B, H, H, d.dh[l] + t * BH, H, 1);
                // attention context
                sk_linear_job(jy[ny++], rseg(dG, l, 0, H, 2 * H), d.B, E, H, dctx(d.dw0, d.dw, l, t), E, 1);
                sk_linear_job(jx[nx++], rseg(dC, l, 1, H, H), d.B, E, H, dctx(d.dw0, d.dw, l, t), E, 1);
                for (int p = 0; p < l; ++p) {  // lower layers' states of the same step (separate buffer: no two jobs share a tile)
                    sk_linear_job(jy[ny++], rseg(dG, l, 0, H + E + p * H, 2 * H), d.B, H, H, d.dhup[p] + (t + 1) * BH, H, 1);
                    sk_linear_job(jx[nx++], rseg(dC, l, 1, H + E + p * H, H), d.B, H, H, d.dhup[p] + (t + 1) * BH, H, 1);
                }
            }
            if (ga.nchain == 0) continue;
            // layer 0's chain (if active) is the last one added; attention + all state updates in one launch
            PL_TRY(traced_att_state_bwd_launch(att_on ? &g : nullptr, ga, att_on ? ga.nchain - 1 : -1, st));
            PL_TRY(launch_jobs(jx, nx, st, full_wgs));
            PL_TRY(launch_jobs(jy, ny, st, full_wgs));
        }
        return 0;
    }

    // ---- bwd8: the K-balanced backward tick (f32 GRU decoders of 2 or 3 layers) ------------------------------------------
    // The tick of bwd() is three dependent launches: attention + state backward (11.1 us at cfg2: a chain of dependent
    // round trips on 64-128 CUs, the rest idle), X (d(rh) and the dC products, K = H: 9.5 us) and Y (the dG products,
    // K = 2H: 14.3 us -- a launch costs ~4.7 us + ~4.8 us per 1024 of its LONGEST K, tools/tick_model.py).  A tick is 672
    // units of 32 x 32 x K1024 work, 2.6 rounds of 256 CUs, so three launches are the minimum -- but they need not be
    // one idle launch, one short and one long.  Here
    //   * every K = 2H product is cut into its update-gate (z) and reset-gate (r) halves, K = H each, writing SEPARATE
    //     buffers that the consumer adds (second / third accumulators of ParrotDecoderDesc): dG_z exists after the state
    //     backward, dG_r only after X, so the z halves move up a launch;
    //   * layer 1 runs TWO ticks ahead of layer 0, so its downward products (into dhup_0 and dw) have a tick of slack;
    //   * those with dG operands ride in the NEXT tick's attention launch as step-GEMM workgroups beside the attention
    //     backward blocks (skinny.hip skb_kernel), the dC ones in Y.
    // Per tick (L = 2, cfg2): S' = 64 attention rows + 64 state rows + 160 GEMM workgroups, X = 256, Y = 256, every K = H:
    // predicted 12.1 + 9.5 + 9.5 = 31.1 us against 34.9 (profiles/r04_tick_model_whatif.txt).
    int lag8(int l) const { return 2 * (d.L - 1 - l); }
    int nticks8() const { return d.T + 2 * (d.L - 1); }
    int bwd8(hipStream_t st) {
        const size_t BH = (size_t)d.B * d.H, BE = (size_t)d.B * d.E;
        const int H = d.H, E = d.E, Q = nticks8();
        for (int q = 0; q < Q; ++q) {
            int tl[PARROT_MAX_LAYERS];
            for (int l = 0; l < d.L; ++l) tl[l] = d.T - 1 - (q - lag8(l));
            const int t0 = tl[0];
            const bool att_on = t0 >= 0 && t0 < d.T;
            AttBwdArgs g{};
            if (att_on) {
                g = att_bwd_args(t0);
                g.dw3 = d.dw0_b + (size_t)(t0 + 1) * BE; g.dw4 = d.dw0_c + (size_t)(t0 + 1) * BE;
                g.dw5 = d.dw_b + (size_t)(t0 + 1) * BE;  g.dw6 = d.dw_c + (size_t)(t0 + 1) * BE;
            }
            // ---- S': state backward of every active layer (+ attention), and the deferred downward products
            GruStateBwdArgs ga;
            ga.nchain = 0; ga.B = d.B; ga.H = H;
            for (int l = d.L - 1; l >= 0; --l) {
                const int t = tl[l];
                if (t < 0 || t >= d.T) continue;
                GruStateBwdChain& c = ga.chain[ga.nchain++];
                c = gru_chain(l, t);
                c.dhx[0] = d.dh_b[l] + (t + 1) * BH;
                c.dhx[1] = (l + 1 < d.L) ? d.dhup_b[l] + (t + 1) * BH : nullptr;
                c.dhx[2] = (l + 1 < d.L) ? d.dhup_c[l] + (t + 1) * BH : nullptr;
            }
            // (L = 3: a tick has 10 / 6 / 11 jobs for S' / X / Y and a launch carries SK_MAXJOB = 9 -- its
            // descriptors travel by value in the 4 KB kernel-argument block --, so the lists are built generously and
            // the overflow is moved: S' -> Y (everything S' multiplies is a tick old), Y -> X for the jobs that do not
            // read what X writes: the dC products and the update-gate halves, `ymov`.)
            constexpr int JCAP = 2 * SK_MAXJOB;
            SkJob js[JCAP], jx[JCAP], jy[JCAP];
            bool ymov[JCAP];
            int ns = 0, nx = 0, ny = 0;
            for (int l = d.L - 1; l >= 1; --l) {  // the dG halves of the step layer l handled one tick ago
                const int s = tl[l] + 1;
                if (s < 0 || s >= d.T) continue;
                const float* dG = d.dG[l] + (size_t)s * 2 * BH;
                for (int p = 0; p < l; ++p) {
                    sk_linear_job(js[ns++], rseg_k(dG, l, 0, H + E + p * H, 2 * H, 0, H), d.B, H, H, d.dhup_b[p] + (s + 1) * BH, H, 1);
                    sk_linear_job(js[ns++], rseg_k(dG, l, 0, H + E + p * H, 2 * H, H, H), d.B, H, H, d.dhup_c[p] + (s + 1) * BH, H, 1);
                }
                sk_linear_job(js[ns++], rseg_k(dG, l, 0, H, 2 * H, 0, H), d.B, E, H, d.dw_b + (size_t)(s + 1) * BE, E, 1);
                sk_linear_job(js[ns++], rseg_k(dG, l, 0, H, 2 * H, H, H), d.B, E, H, d.dw_c + (size_t)(s + 1) * BE, E, 1);
            }
            // ---- X: d(r*h) (epilogue: dG_r, dh_prev += d(rh) * r) and the update-gate half of dG -> dh_prev (own buffer)
            // ---- Y: the reset-gate half of dG -> dh_prev, layer 0's context shares, the upper layers' dC shares downward
            for (int l = d.L - 1; l >= 0; --l) {
                const int t = tl[l];
                if (t < 0 || t >= d.T) continue;
                const float* dG = d.dG[l] + (size_t)t * 2 * BH;
                const float* dC = d.dC[l] + t * BH;
                rh_job(jx[nx++], l, t);
                sk_linear_job(jx[nx++], rseg_k(dG, l, 0, 0, 2 * H, 0, H), d.B, H, H, d.dh_b[l] + t * BH, H, 0);
                ymov[ny] = false; sk_linear_job(jy[ny++], rseg_k(dG, l, 0, 0, 2 * H, H, H), d.B, H, H, d.dh[l] + t * BH, H, 1);
                ymov[ny] = true;  sk_linear_job(jy[ny++], rseg(dC, l, 1, H, H), d.B, E, H, dctx(d.dw0, d.dw, l, t), E, 1);
                if (l == 0) {
                    ymov[ny] = true;  sk_linear_job(jy[ny++], rseg_k(dG, 0, 0, H, 2 * H, 0, H), d.B, E, H, d.dw0_b + (size_t)t * BE, E, 0);
                    ymov[ny] = false; sk_linear_job(jy[ny++], rseg_k(dG, 0, 0, H, 2 * H, H, H), d.B, E, H, d.dw0_c + (size_t)t * BE, E, 0);
                }
                for (int p = 0; p < l; ++p) {
                    ymov[ny] = true;
                    sk_linear_job(jy[ny++], rseg(dC, l, 1, H + E + p * H, H), d.B, H, H, d.dhup[p] + (t + 1) * BH, H, 1);
                }
            }
            while (ns > SK_MAXJOB) { ymov[ny] = true; jy[ny++] = js[--ns]; }  // (a tick old: movable further, too)
            for (int i = ny - 1; i >= 0 && ny > SK_MAXJOB && nx < SK_MAXJOB; --i)
                if (ymov[i]) {
                    jx[nx++] = jy[i];
                    for (int k2 = i; k2 + 1 < ny; ++k2) { jy[k2] = jy[k2 + 1]; ymov[k2] = ymov[k2 + 1]; }
                    --ny;
                }
            if (ns > SK_MAXJOB || nx > SK_MAXJOB || ny > SK_MAXJOB) return PARROT_ERR_BADARG;
            if (ga.nchain > 0) {
                const int l0c = att_on ? ga.nchain - 1 : -1;
                if (ns > 0) PL_TRY(traced_bwd_hetero_launch(att_on ? &g : nullptr, ga, l0c, js, ns, st));
                else PL_TRY(traced_att_state_bwd_launch(att_on ? &g : nullptr, ga, l0c, st));
            } else if (ns > 0) {
                PL_TRY(launch_jobs(js, ns, st, full_wgs));
            }
            if (nx > 0) PL_TRY(launch_jobs(jx, nx, st, full_wgs));
            if (ny > 0) PL_TRY(launch_jobs(jy, ny, st, full_wgs));
        }
        return 0;
    }

    // ---- schedule 3, backward: the mirror of fwd_skew (upper layers lead by a chunk; hoist_bwd after a layer's chunk) ----
    int bwd_skew(hipStream_t st) {
        const size_t BH = (size_t)d.B * d.H, BE = (size_t)d.B * d.E;
        const int H = d.H, E = d.E;
        const int C = ceil_div(d.T, chunk);
        for (int sc = 0; sc < C + d.L - 1; ++sc) {
            int cl[PARROT_MAX_LAYERS];
            for (int l = 0; l < d.L; ++l) cl[l] = C - 1 - (sc - (d.L - 1 - l));  // upper layers lead
            for (int s = chunk - 1; s >= 0; --s) {
                int tl[PARROT_MAX_LAYERS];
                for (int l = 0; l < d.L; ++l) {
                    const int t = cl[l] * chunk + s;
                    tl[l] = (cl[l] >= 0 && cl[l] < C && t < d.T) ? t : -1;
                }
                const int t0 = tl[0];
                AttBwdArgs g{};
                if (t0 >= 0) {
                    g = att_bwd_args(t0);
                    if (d.cell == 1) PL_TRY(att_bwd_launch(g, st));
                }
                GruStateBwdArgs ga;
                ga.nchain = 0; ga.B = d.B; ga.H = H;
                SkJob jx[PARROT_MAX_LAYERS], jy[2 * PARROT_MAX_LAYERS];
                int nx = 0, ny = 0;
                for (int l = d.L - 1; l >= 0; --l) {  // the hoisted projections' shares are hoist_bwd's: only the own block here
                    const int t = tl[l];
                    if (t < 0) continue;
                    if (d.cell == 1) {
                        const LstmStateBwdChain c = lstm_chain(l, t);
                        PL_TRY(lstm_state_bwd_launch(c.dh, c.dh2, c.dc, c.gates, c.c_prev, c.c_new, c.dP, d.B, H, st));
                        sk_linear_job(jy[ny++], rseg(c.dP, l, 0, 0, 4 * H), d.B, H, H, d.dh[l] + t * BH, H, 1);
                        if (l == 0) sk_linear_job(jy[ny++], rseg(c.dP, 0, 0, H, 4 * H), d.B, E, H, d.dw0 + (size_t)t * BE, E, 1);
                        continue;
                    }
                    ga.chain[ga.nchain++] = gru_chain(l, t);
                    rh_job(jx[nx++], l, t);
                    const float* dG = d.dG[l] + t * 2 * BH;
                    const float* dC = d.dC[l] + t * BH;
                    sk_linear_job(jy[ny++], rseg(dG, l, 0, 0, 2 * H), d.B, H, H, d.dh[l] + t * BH, H, 1);
                    if (l == 0) {  // layer 0's context share: the dG and dC products as the two segments of one job
                        SkJob& j = jy[ny++];
                        sk_linear_job(j, rseg(dG, 0, 0, H, 2 * H), d.B, E, H, d.dw0 + (size_t)t * BE, E, 1);
                        j.seg[j.nseg++] = rseg(dC, 0, 1, H, H);
                    }
                }
                if (d.cell == 0) {
                    if (ga.nchain == 0) continue;
                    PL_TRY(traced_att_state_bwd_launch(t0 >= 0 ? &g : nullptr, ga, t0 >= 0 ? ga.nchain - 1 : -1, st));
                    PL_TRY(launch_jobs(jx, nx, st));
                }
                if (ny > 0) PL_TRY(launch_jobs(jy, ny, st));
            }
            for (int l = 1; l < d.L; ++l) {
                const int c = cl[l];
                if (c >= 0 && c < C) PL_TRY(hoist_bwd(l, c * chunk, (c + 1) * chunk < d.T ? (c + 1) * chunk : d.T, st));
            }
        }
        return 0;
    }

    // ---- schedule 4: persistent phase machine for the forward scan (persist.h) ---------------------------------
    // Units per step t: layer 0: G0 = gates over [h0[t]; w[t]], C0 = candidate over [r*h0; w[t]], ATT (one per batch
    // row); layer l >= 1: IG_l / IC_l = the projections of [w[t+1]; h_0[t+1] .. h_{l-1}[t+1]] into the layer's gates /
    // candidate (written to pre-activation buffers), G_l / C_l = the recurrent products over h_l[t] / r*h_l.
    // Tick q runs slot 0: G0(q), G_l(q - 2l);  slot 1: C0(q), C_l(q - 2l), IC_l(q - 2l + 1);  slot 2: ATT(q),
    // IG_l(q - 2l + 1).  Every unit's inputs were published at least one barrier earlier (see the lag arithmetic in
    // DESIGN.md).  Units are spread over the workgroups greedily; a unit's weight slab stays in the workgroup's LDS
    // for the whole window when it fits (critical recurrent units first), otherwise it is streamed.
    // The carve-up of the workspace, the descriptors, the capacity checks, placement and upload are PmBuilder's
    // (pm_builder.h, shared with the decode planners); build_persist says which slabs and units there are.
    enum { PERSIST_MAXPIECES = 4, TR_SLOTS = 3, TR_MAXU = 3 };
    static long long persist_floats(const ParrotDecoderDesc& d, int nwg) {
        const long long rows = pm_rows(d.B);
        long long n = pm_header_floats((long long)TR_SLOTS * nwg * TR_MAXU);
        n += 2 * (long long)(d.T + 1) * rows * (d.H + d.E);                       // XG0, XC0
        for (int l = 1; l < d.L; ++l)
            n += 2 * (long long)(d.T + 1) * rows * d.H + (long long)d.T * rows * (d.E + l * d.H);  // XG_l, XC_l, XI_l
        for (int l = 1; l < d.L; ++l) n += (long long)d.T * d.B * 3 * d.H * PERSIST_MAXPIECES / (l == 1 ? 2 : 1);  // partials
        return n + 1024;
    }
    static bool persist_eligible(const ParrotDecoderDesc& d) {
        if (d.cell != 0 || d.layer_norm || d.bf16 || d.B > 64 || (d.H % 16) || (d.E % 16) || d.U > PM_ATT_MAXU ||
            d.A > PM_ATT_MAXA || d.T < 1)
            return false;
        for (int l = 0; l < d.L; ++l)
            if (!d.Wg_f[l] || !d.Wc_f[l]) return false;
        return pm_max_workgroups() >= 64;
    }

    int build_persist() {
        persist_ok = false;
        if (!persist_eligible(d) || !tiled || !d.persist_ws) return 0;
        const int nwg = pm_max_workgroups();
        if (d.persist_ws_floats < persist_floats(d, nwg)) return 0;
        const int H = d.H, E = d.E, B = d.B, L = d.L, T = d.T;
        const long long BH = (long long)B * H;
        PmBuilder pb(pm_prog, false, d.persist_ws, d.persist_ws_floats, B, nwg, TR_SLOTS, TR_MAXU);
        const long long rows = pb.rows;
        // activation slabs (fragment-major, one per consumer kind and step):
        //   XG[l][t] = A operand of G_l(t):  l = 0: [h_0[t] ; w[t]],  l >= 1: [h_l[t]]
        //   XC[l][t] = A operand of C_l(t):  l = 0: [r*h_0 ; w[t]],   l >= 1: [r*h_l]
        //   XI[l][t] = A operand of IG_l(t) / IC_l(t), l >= 1: [w[t+1] ; h_0[t+1] ; .. ; h_{l-1}[t+1]]
        float* XG[PARROT_MAX_LAYERS];
        float* XC[PARROT_MAX_LAYERS];
        float* XI[PARROT_MAX_LAYERS] = {nullptr, nullptr, nullptr};
        long long kx[PARROT_MAX_LAYERS], ki[PARROT_MAX_LAYERS] = {0, 0, 0};
        for (int l = 0; l < L; ++l) {
            kx[l] = l == 0 ? H + E : H;
            XG[l] = pb.take((long long)(T + 1) * rows * kx[l]);
            XC[l] = pb.take((long long)(T + 1) * rows * kx[l]);
            if (l >= 1) {
                ki[l] = E + (long long)l * H;
                XI[l] = pb.take((long long)T * rows * ki[l]);
            }
        }
        pb.fm_end();
        // Input projections of the layers l >= 1 are cut into pieces (K ranges of the XI slab) that write separate
        // partial pre-activation buffers; the consuming recurrent unit adds them.  Pieces: the w rows, then per lower
        // layer its H rows (one piece per lower layer: halves of them measured slower at cfg2 -- every unit carries
        // ~3.5 us of fixed latency).
        float* pre[PARROT_MAX_LAYERS][2][PERSIST_MAXPIECES];
        memset(pre, 0, sizeof(pre));
        float* const pre_begin = pb.mark();
        for (int l = 1; l < L; ++l)
            for (int g = 0; g < 2; ++g)
                for (int q = 0; q < (l == 1 ? PERSIST_MAXPIECES / 2 : PERSIST_MAXPIECES); ++q)
                    pre[l][g][q] = pb.take((long long)T * B * (g == 0 ? 2 * H : H));
        float* const pre_end = pb.mark();
        if (pb.failed) return 0;

        auto seq_on = [&](int l, const float* p) { return p && ((d.seq_init >> l) & 1); };
        for (int l = 0; l < L; ++l) {
            const int Kl = krows(l), nchK = Kl / 16;
            for (int g = 0; g < 2; ++g) {                      // g = 0: gates (2H wide), 1: candidate (H wide)
                const int wd = g == 0 ? 2 * H : H;
                const float* Wf = g == 0 ? d.Wg_f[l] : d.Wc_f[l];
                const float* bias = g == 0 ? d.bg[l] : d.bc[l];
                float* sq = g == 0 ? d.seq_g[l] : d.seq_c[l];
                for (int ct = 0; ct < wd / 16; ++ct) {
                    // recurrent unit (layer 0: the whole product)
                    PmReq q = pb.gemm(g, g == 0 ? XG[l] : XC[l], kx[l], 0, (int)kx[l], 2 * l);
                    PmUnit& u = q.u;
                    u.W = Wf + (size_t)ct * nchK * 256;
                    if (l == 0) {
                        u.bias = bias ? bias + 16 * ct : nullptr;
                        if (seq_on(l, sq)) pb.add_operand(u, pm_rm(sq + 16 * ct, (long long)B * wd, wd));
                    }
                    if (g == 0) {
                        u.epi = PM_EPI_GATES;
                        u.rtile = 16 * ct >= H;
                        if (!u.rtile) {
                            u.o1 = pm_rm(d.z[l] + 16 * ct, BH, H);
                        } else {
                            const int j0 = 16 * ct - H;
                            u.o2 = pm_rm(d.r[l] + j0, BH, H);
                            u.e0 = pm_rm(d.h[l] + j0, BH, H);
                            u.out = pm_rm(d.rh[l] + j0, BH, H);
                            pb.add_dst(u, pb.dst(XC[l], 0, kx[l], j0 / 16));
                        }
                    } else {
                        u.epi = PM_EPI_CAND;
                        u.e0 = pm_rm(d.h[l] + 16 * ct, BH, H);
                        u.e1 = pm_rm(d.z[l] + 16 * ct, BH, H);
                        u.o1 = pm_rm(d.c[l] + 16 * ct, BH, H);
                        u.out = pm_rm(d.h[l] + BH + 16 * ct, BH, H);
                        pb.add_dst(u, pb.dst(XG[l], 1, kx[l], ct));                  // h_l[t+1] for G_l(t+1)
                        for (int m2 = l + 1; m2 < L; ++m2)                            // ... and for the layers above
                            pb.add_dst(u, pb.dst(XI[m2], 0, ki[m2], E / 16 + l * (H / 16) + ct));
                    }
                    // input projection of the layer (l >= 1), one tick ahead of its consumer: piece 0 = the w rows,
                    // piece 1 + j = the rows of h_j
                    for (int pi = 0; l >= 1 && pi <= l; ++pi) {
                        const int c0 = pi == 0 ? 0 : E / 16 + (pi - 1) * (H / 16), K = pi == 0 ? E : H;
                        PmReq qi = pb.gemm(g == 0 ? 2 : 1, XI[l], ki[l], c0, K, 2 * l - 1);
                        PmUnit& v = qi.u;
                        v.W = Wf + ((size_t)ct * nchK + H / 16 + c0) * 256;
                        if (pi == 0) {
                            v.bias = bias ? bias + 16 * ct : nullptr;
                            if (seq_on(l, sq)) pb.add_operand(v, pm_rm(sq + 16 * ct, (long long)B * wd, wd));
                        }
                        v.epi = PM_EPI_LINEAR;
                        v.out = pm_rm(pre[l][g][pi] + 16 * ct, (long long)B * wd, wd);
                        pb.add_operand(u, v.out);
                        qi.crit = 0;
                        pb.push(qi);
                    }
                    pb.push(q);
                }
            }
        }
        pb.att_rows(2, 0);

        pb.att_common(d, d.h[0]);
        PmAtt& a = pm_prog.att;
        a.b = d.b; a.sup = d.att_sup; a.dense = sw_att_dense();
        pb.add_wdst(pb.dst(XG[0], 1, kx[0], H / 16));   // w[t+1] for G_0(t+1) and C_0(t+1) ...
        pb.add_wdst(pb.dst(XC[0], 1, kx[0], H / 16));
        for (int l = 1; l < L; ++l) pb.add_wdst(pb.dst(XI[l], 0, ki[l], 0));  // ... and for the layers above
        for (int l = 0; l < L; ++l) pb.add_init(d.h[l], H, H, XG[l], kx[l], 0);  // states entering the window (slot 0)
        pb.add_init(d.w, E, E, XG[0], kx[0], H / 16);
        pb.add_init(d.w, E, E, XC[0], kx[0], H / 16);
        // dataflow mode: everything a unit reads from another workgroup starts EMPTY (slot 0 of the histories is the
        // caller's: the states entering the window)
        pm_prog.dataflow = sw_pm_dataflow(0);
        pb.fill_fm();
        pb.add_fill(pre_begin, (long long)(pre_end - pre_begin));
        for (int l = 0; l < L; ++l) {
            pb.add_fill(d.h[l] + BH, (long long)T * BH);
            pb.add_fill(d.z[l], (long long)T * BH);
        }
        persist_ok = pb.finish(T, T + 2 * (L - 1));
        return 0;
    }
    int persist_status() const { return persist_ok ? pm_status(pm_prog) : 0; }

    // ---- resolve(): which schedule and which backward tick this descriptor runs ------------------------------------------
    // Called once, by parrot_decoder_create on the copied descriptor.  Returns 0, or the error the create call returns (the
    // caller deletes the plan).  Nothing after it changes what the plan runs: enqueue(), has_seq() and the C accessors
    // (parrot_decoder_schedule, _backward_tick, _writes_bf16_grads, _is_persistent) read what is decided here.
    int resolve() {
        const int B = d.B, H = d.H, E = d.E, L = d.L;
        esplit = att_default_esplit(B, E);
        s5_w_in_step = env_int("PARROT_S5_WSTEP", 1) != 0;
        const int c = env_int("PARROT_CHUNK", 0);  // (tests: several chunks and a ragged last one on short windows)
        if (c > 0) chunk = c;

        // -- weight operands: the fragment-major copies when the caller gave all of them
        tiled = (H % 16 == 0) && (E % 16 == 0);
        for (int l = 0; l < L; ++l) {
            if (!d.Wg_f[l] || !d.Wg_r[l]) tiled = false;
            if (d.cell == 0 && (!d.Wc_f[l] || !d.Wc_r[l])) tiled = false;
        }
        // bf16 operands exist only as fragment-major copies; 32-deep K chunks
        if (d.bf16 && (!tiled || d.layer_norm || (H % 32) || (E % 32))) return PARROT_ERR_BADARG;

        // -- the forward schedule
        int want = env_int("PARROT_SCHEDULE", -1);
        bool pipe_ok = L >= 2;  // the upper layers have the seq buffers the input projections of 3 and 5 write
        for (int l = 1; l < L; ++l)
            if (!d.seq_g[l] || (d.cell == 0 && !d.seq_c[l])) pipe_ok = false;
        // 4 = persistent forward scan, opt-in: measured at cfg2 it only matches the launch schedules.  Everything
        // it does not cover -- the backward scan, LSTM layers, layer_norm, B > 64 -- runs on the launch schedule chosen below.
        const bool want_persist = want == 4;
        if (want_persist) want = -1;
        if (want < 0) {
            // default: the balanced wavefront (5) where it pays -- GRU layers, L >= 2, no layer_norm; measured at cfg2:
            // forward scan 29.2 -> 25.2 ms
            // GRU stacks, f32 or bf16 operands (cfg2: 82.7 -> 74.6 ms f32, 59.8 -> 54.0 ms bf16; 3 layers 122.5 -> 115.0).
            // LSTM stacks stay on schedule 0 (5 covers them, opt-in): their tick is ONE fused launch of > 1000 workgroups,
            // bound by total work rather than by its longest K, and cutting it in two only adds fixed cost -- cfg4 bf16
            // 118.9 vs 127.5 ms (the wide kernel has ~10 us of fixed cost per launch), cfg4 f32 256.5 vs 265.4 ms.
            want = (pipe_ok && d.cell == 0 && !d.layer_norm) ? 5 : 0;
            // LSTM stacks with bf16 operands (BASELINE configs[3]): the attention inside the tick's one launch (7), where
            // the wide step kernel takes the launch (checked below)
            if (d.cell == 1 && d.bf16 && !d.layer_norm) want = 7;
        }
        if (d.layer_norm && L >= 2 && want < 2) want = 3;  // the in-scan normalisations need the hoisted projections
        if (want != 0 && want != 3 && want != 5 && want != 7) want = 0;  // (1, 2 and 6: measured losers, numbers in DESIGN.md 3.2)
        if (want >= 2 && want != 7 && !pipe_ok) want = 0;
        if (want == 7 && d.cell != 1) want = pipe_ok ? 5 : 0;  // one launch per tick: LSTM layers
        if (want >= 5 && d.layer_norm) want = 0;
        // 7 with bf16 operands: only the wide step kernel takes a launch with a waiting job (skinny.hip wk_try_launch): every
        // launch of the scan must qualify, the first tick's (layer 0 alone) included.  f32 operands run on ska_kernel (and
        // reach schedule 7 only when PARROT_SCHEDULE asks for it).
        if (want == 7 && !(tiled && B <= 64 && (!d.bf16 || sk_wide_takes(B, 4 * H, H, E)))) want = 0;
        schedule = want;

        // -- schedule 7: the arrival counters, and with bf16 operands the backward tick as one launch too (wkb_kernel)
        if (schedule == 7) {
            if (hipMalloc(&att_flags, sizeof(unsigned) * (size_t)(d.T + 2)) != hipSuccess) {
                if (!env_set("PARROT_TRACE_ONLY")) return PARROT_ERR_BADARG;
                (void)hipGetLastError();  // (schedule tracing on a box without a GPU: placeholder addresses)
                att_flags = reinterpret_cast<unsigned*>((uintptr_t)0x1000);
                flags_fake = true;
            }
            if (d.bf16) {
                const size_t words = (size_t)4 * (d.T + L);
                if (flags_fake) bwd_flags = reinterpret_cast<unsigned*>((uintptr_t)0x100000);
                else if (hipMalloc(&bwd_flags, sizeof(unsigned) * words) != hipSuccess) return PARROT_ERR_BADARG;
                bwd_fused = true;
            }
        }
        // -- bf16 LSTM stacks: the backward products in two K halves, when the second accumulators are there
        if (d.cell == 1 && d.bf16 && tiled) {
            bool have = d.dw_b && d.dw0_b && B <= 64 && sk_wide_takes(B, 4096, H, E) && (4 * H) % 128 == 0;
            for (int l = 0; l < L; ++l)
                if (!d.dh_b[l] || (l + 1 < L && !d.dhup_b[l])) have = false;
            bwd_ksplit = have;
        }
        // -- schedule 4: persist_ok stays false when the shape / workspace does not qualify
        if (want_persist && d.cell == 0 && !d.layer_norm && !d.bf16) build_persist();
        // -- the K-balanced backward tick (bwd8): f32 GRU decoders of 2 or 3 layers with fragment-major weights and all
        // accumulators (PARROT_BWD_HETERO=0 opts out).  Schedule 3 runs its own backward (bwd_skew), whatever it is given.
        {
            bool ok = d.cell == 0 && (L == 2 || L == 3) && !d.bf16 && !d.layer_norm && tiled && B <= 64 && schedule != 3 &&
                      d.dw_b && d.dw_c && d.dw0_b && d.dw0_c && env_int("PARROT_BWD_HETERO", 1) != 0;
            for (int l = 0; l < L; ++l)
                if (!d.dh_b[l] || (l + 1 < L && (!d.dhup_b[l] || !d.dhup_c[l]))) ok = false;
            bwd_hetero = ok;
        }
        // -- layer_norm above layer 0 runs on the hoisted projections only, and needs its buffers
        if (d.layer_norm && L >= 2) {
            bool ok = schedule >= 2 && schedule != 7;
            for (int l = 1; l < L && ok; ++l)
                for (int j = 0; j < l; ++j) {
                    const int pj = l * PARROT_MAX_LAYERS + j;
                    if (!d.ln_yg[pj] || !d.ln_sg[pj] || !d.ln_bg[pj]) ok = false;
                    if (d.cell == 0 && (!d.ln_yc[pj] || !d.ln_sc[pj] || !d.ln_bc[pj])) ok = false;
                }
            if (!ok) return PARROT_ERR_BADARG;
        }
        return 0;
    }
};

}  // namespace

extern "C" {


int parrot_gru_seq_create(const ParrotGruSeqDesc* desc, void** plan) { PH_ENTRY();
    if (!desc || !plan || desc->T < 1 || desc->B < 1 || desc->H < 1 || desc->nchain < 1 || desc->nchain > 4)
        return PARROT_ERR_BADARG;
    GruSeqPlan* p = new (std::nothrow) GruSeqPlan();
    if (!p) return PARROT_ERR_BADARG;
    p->d = *desc;
    p->use_graph = desc->use_graph;
    p->setup_rowwise();
    *plan = p;
    return 0;
}
int parrot_gru_seq_fwd(void* plan, void* stream) { PH_ENTRY(); return static_cast<PlanBase*>(plan)->run(0, (hipStream_t)stream); }
int parrot_gru_seq_bwd(void* plan, void* stream) { PH_ENTRY(); return static_cast<PlanBase*>(plan)->run(1, (hipStream_t)stream); }
int parrot_gru_seq_destroy(void* plan) { PH_ENTRY();
    delete static_cast<PlanBase*>(plan);
    return 0;
}
int parrot_gru_seq_route(void* plan, int* info4) {  // (no HIP call: the plan's own record)
    if (!plan || !info4) return PARROT_ERR_BADARG;
    const GruSeqPlan* p = static_cast<GruSeqPlan*>(plan);
    info4[0] = p->rowwise ? 1 : 0;
    info4[1] = p->rowwise ? p->waves : 0;
    info4[2] = p->rowwise ? p->d.H / 16 : 0;
    info4[3] = p->reason;
    return 0;
}
int parrot_gru_seq_rowwise_supported(int T, int B, int H, int nchain) { return rowgru_supported(T, B, H, nchain) ? 1 : 0; }

int parrot_lstm_seq_create(const ParrotLstmSeqDesc* desc, void** plan) { PH_ENTRY();
    if (!desc || !plan || desc->T < 1 || desc->B < 1 || desc->H < 4 || (desc->H & 3)) return PARROT_ERR_BADARG;
    LstmSeqPlan* p = new (std::nothrow) LstmSeqPlan();
    if (!p) return PARROT_ERR_BADARG;
    p->d = *desc;
    p->use_graph = desc->use_graph;
    *plan = p;
    return 0;
}
int parrot_lstm_seq_fwd(void* plan, void* stream) { PH_ENTRY(); return static_cast<PlanBase*>(plan)->run(0, (hipStream_t)stream); }
int parrot_lstm_seq_bwd(void* plan, void* stream) { PH_ENTRY(); return static_cast<PlanBase*>(plan)->run(1, (hipStream_t)stream); }
int parrot_lstm_seq_destroy(void* plan) { PH_ENTRY();
    delete static_cast<PlanBase*>(plan);
    return 0;
}

int parrot_decoder_create(const ParrotDecoderDesc* desc, void** plan) { PH_ENTRY();
    if (!desc || !plan || desc->T < 1 || desc->B < 1 || bad_dims(desc->L)) return PARROT_ERR_BADARG;
    DecoderPlan* p = new (std::nothrow) DecoderPlan();
    if (!p) return PARROT_ERR_BADARG;
    p->d = *desc;
    p->use_graph = desc->use_graph;
    const int rc = p->resolve();
    if (rc != 0) {
        delete p;
        return rc;
    }
    *plan = p;
    return 0;
}
long long parrot_decoder_persist_floats(const ParrotDecoderDesc* desc) { PH_ENTRY();
    if (!desc || !DecoderPlan::persist_eligible(*desc)) return 0;
    return DecoderPlan::persist_floats(*desc, pm_max_workgroups());
}
int parrot_decoder_status(void* plan) { PH_ENTRY(); return plan ? static_cast<DecoderPlan*>(plan)->persist_status() : PARROT_ERR_BADARG; }

int parrot_decoder_is_persistent(void* plan) { return static_cast<DecoderPlan*>(plan)->persist_ok ? 1 : 0; }
int parrot_decoder_schedule(void* plan) { return plan ? static_cast<DecoderPlan*>(plan)->schedule : -1; }
int parrot_decoder_backward_tick(void* plan) { return plan ? (static_cast<DecoderPlan*>(plan)->bwd_hetero ? 8 : (static_cast<DecoderPlan*>(plan)->bwd_fused ? 7 : 0)) : -1; }
int parrot_decoder_writes_bf16_grads(void* plan) {
    const DecoderPlan* p = static_cast<const DecoderPlan*>(plan);
    if (!p || !p->bwd_fused) return 0;
    for (int l = 0; l < p->d.L; ++l)
        if (!p->d.dG16[l]) return 0;
    return 1;
}
long long parrot_decoder_trace_jobs(void* plan, int which, long long* out, long long cap) { PH_ENTRY();
    if (!plan || which < 0 || which > 1) return -PARROT_ERR_BADARG;
    std::vector<TraceRec> recs;
    std::vector<TraceJob> jobs;
    const int rc = static_cast<DecoderPlan*>(plan)->trace(which, recs, &jobs);
    if (rc != 0) return -(long long)rc;
    const long long n = (long long)jobs.size();
    if (out)
        for (long long i = 0; i < n && i < cap; ++i) {
            out[6 * i] = jobs[i].launch; out[6 * i + 1] = jobs[i].job; out[6 * i + 2] = jobs[i].M;
            out[6 * i + 3] = jobs[i].N; out[6 * i + 4] = jobs[i].Kmax_seg_sum; out[6 * i + 5] = jobs[i].epi;
        }
    return n;
}
long long parrot_decoder_trace(void* plan, int which, long long* out, long long cap) { PH_ENTRY();
    if (!plan || which < 0 || which > 1) return -PARROT_ERR_BADARG;
    std::vector<TraceRec> recs;
    const int rc = static_cast<DecoderPlan*>(plan)->trace(which, recs);
    if (rc != 0) return -(long long)rc;
    const long long n = (long long)recs.size();
    if (out)
        for (long long i = 0; i < n && i < cap; ++i) {
            out[5 * i] = recs[i].launch; out[5 * i + 1] = recs[i].job; out[5 * i + 2] = recs[i].kind;
            out[5 * i + 3] = recs[i].lo; out[5 * i + 4] = recs[i].hi;
        }
    return n;
}

int parrot_decoder_seq_fwd(void* plan, void* stream) { PH_ENTRY(); return static_cast<PlanBase*>(plan)->run(0, (hipStream_t)stream); }
int parrot_decoder_seq_bwd(void* plan, void* stream) { PH_ENTRY(); return static_cast<PlanBase*>(plan)->run(1, (hipStream_t)stream); }
int parrot_decoder_destroy(void* plan) { PH_ENTRY();
    delete static_cast<PlanBase*>(plan);
    return 0;
}

int parrot_plan_last_error(void* plan) { PH_ENTRY(); return plan ? static_cast<PlanBase*>(plan)->last_error : PARROT_ERR_BADARG; }

}  // extern "C"

// The decode loop of Parrot.sample_model_fun (model.py:882-1057) as a plan: per-step launches in one hipGraph, or the
// whole loop as ONE resident kernel on the persistent phase machine (persist.h) -- 2L + 3 whole-K phases
// (build_persist_whole), 2L + 2 phases with every product cut along K by the age of its operands, 2L + 1 with the fed-back
// frame out of the step's dependency chain (both build_persist_pieces); LSTM stacks: L + 2 whole-K phases
// (build_persist_lstm); with a GMM head (PARROT_PM_GMM=1) the two whole-K programs end in a composed head phase and a
// sampling phase instead (gmm_eligible).  SamplePlan::plan_persist picks the program (SamplePlan::Program), for real and
// for dry runs alike.  The three planners speak one vocabulary: the slabs of a program and who writes into them (PmSlabs,
// SamplePlan::carve), one emitter per unit kind that pushes the units AND the kind's symbolic-replay meta from the same
// operands (gate_tiles, cand_tiles, linear_tiles, att_rows, head_phases), one tail; a planner itself only says which
// kinds run in which phase on which chunks.  Underneath, the shared builder (pm_builder.h) carves the workspace within
// its bounds, checks the table capacities, places, digests and uploads.  Then the per-step launch path and the
// parrot_sample_* entry points.
#include "pm_builder.h"
#include "switches.h"

namespace {

// ----------------------------------------------------------------------------- planner vocabulary
// A product cut along K (build_persist_pieces): a group is one product of the step, a piece a chunk range of its slab.
struct PmPiece {
    int c0, nch, gp;  // chunk range of the slab; position (phase index over two ticks) after which the operand exists
    bool crit;
    int lag, slot, pbuf;
};
struct PmGroup {
    int kind, l, slot, N, res;  // kind 0 gates, 1 candidate, 2 output, 3 x_pre (fbc); res = checker resource id of the slab
    int glag;                   // the group's critical unit runs `glag` ticks after the step's other main units
    long long ks;
    std::vector<PmPiece> pc;
};
// The symbolic replay's view of a program: per unit kind what it reads and writes, slabs by chunk, histories as one
// element per step.
struct PmAccess { int res, dstep, c0, nch; };
struct PmMeta { int lag, slot; std::vector<PmAccess> rd, wr; };
enum { RES_XG = 10, RES_XC = 20, RES_XR = 30, RES_XO = 31, RES_RO = 32, RES_H = 40, RES_Z = 50, RES_X = 60, RES_KAPPA = 61, RES_XPRE = 62, RES_PP = 63,
       RES_HEAD = 64, RES_C = 70, RES_PART = 100 };
PmAccess pm_acc(int res, int dstep, int c0, int nch) { PmAccess a; a.res = res; a.dstep = dstep; a.c0 = c0; a.nch = nch; return a; }

// What the units of one kind read: chunks [c0, c0 + nch) of one slab (K = ks per step, `res` in the replay), in phase
// `slot`, `lag` ticks behind.
struct PmIn { int slot, lag; const float* slab; long long ks; int res, c0, nch; };
// One place the result of a unit kind goes: column tile ct -> chunk c0 + ct of the slab of step t + dstep.  A unit's
// destination list and its meta's write list are both made from these (add_tos / wr_tos), so they cannot drift apart.
struct PmTo { const float* slab; long long ks; int res, dstep, c0; };
// A row-major [B, N] buffer that a unit adds in its epilogue and the replay must find written: a partial sum, x_pre.
struct PmPart { float* buf; int res; };

// The slabs and histories of a decode program, in workspace order (SamplePlan::carve), and who writes what into them.
struct PmSlabs {
    int L = 0, hc = 0, ec = 0;                        // layers; chunks of a state / of the attention's w
    float* XG[PARROT_MAX_LAYERS] = {};                // gate slab of layer l (LSTM: the layer's only slab)
    float* XC[PARROT_MAX_LAYERS] = {};                // candidate slab (GRU)
    long long kx[PARROT_MAX_LAYERS] = {};
    int fbch[PARROT_MAX_LAYERS] = {};                 // first of the four chunks of the fed-back frame in layer l's slabs; -1: none
    float* XR = nullptr;                              // [h_0[t+1] .. h_{L-1}[t+1] ; w[t+1]]
    long long kr = 0;
    float* XO = nullptr;                              // readout[t] (whole-K GRU with an MSE head)
    float* h[PARROT_MAX_LAYERS] = {};                 // row-major histories: states [S + 1],
    float* z[PARROT_MAX_LAYERS] = {};                 // update gates [S] (GRU),
    float* c[PARROT_MAX_LAYERS] = {};                 // cells [S + 1] (LSTM),
    float *ro_hist = nullptr, *b_hist = nullptr, *head = nullptr;  // readout, attention b, GMM head [S]

    template <class F>
    void each_slab(int l, F f) const {  // every slab of layer l
        f(XG[l], RES_XG + l);
        if (XC[l]) f(XC[l], RES_XC + l);
    }
    // h_l[t+1]: the layer's own gate slab of the next step, every later layer's slabs, the readout's slab
    std::vector<PmTo> state_tos(int l) const {
        std::vector<PmTo> v = {{XG[l], kx[l], RES_XG + l, 1, 0}};
        for (int m = l + 1; m < L; ++m) each_slab(m, [&](const float* s, int res) { v.push_back({s, kx[m], res, 0, hc + ec + l * hc}); });
        v.push_back({XR, kr, RES_XR, 0, l * hc});
        return v;
    }
    // w[t+1] (attention): layer 0 reads it in the next step, the later layers and the readout in this one
    std::vector<PmTo> w_tos() const {
        std::vector<PmTo> v;
        for (int l = 0; l < L; ++l) each_slab(l, [&](const float* s, int res) { v.push_back({s, kx[l], res, l == 0 ? 1 : 0, hc}); });
        v.push_back({XR, kr, RES_XR, 0, L * hc});
        return v;
    }
    // x[t+1] (63 columns, padded to 64): the fed-back chunks of the next step
    std::vector<PmTo> frame_tos() const {
        std::vector<PmTo> v;
        for (int l = 0; l < L; ++l)
            if (fbch[l] >= 0) each_slab(l, [&](const float* s, int res) { v.push_back({s, kx[l], res, 1, fbch[l]}); });
        return v;
    }
};
void add_tos(PmBuilder& pb, PmUnit& u, const std::vector<PmTo>& tos, int ct) {
    for (const PmTo& t : tos) pb.add_dst(u, pb.dst(t.slab, t.dstep, t.ks, t.c0 + ct));
}
void wr_tos(PmMeta& m, const std::vector<PmTo>& tos, int ntiles) {
    for (const PmTo& t : tos) m.wr.push_back(pm_acc(t.res, t.dstep, t.c0, ntiles));
}

// symbolic replay over S steps: 0 = every read finds its value written in an earlier phase and nothing is written twice
int check_pieces(const std::vector<PmMeta>& metas, const std::vector<PmAccess>& init, int n_slots, int S,
                        int n_ticks) {
    std::vector<std::array<int, 3>> written;  // (res, step, chunk), kept sorted
    auto has = [&](int r, int t, int c) {
        const std::array<int, 3> k = {r, t, c};
        return std::binary_search(written.begin(), written.end(), k);
    };
    auto put = [&](int r, int t, int c) {
        const std::array<int, 3> k = {r, t, c};
        auto it = std::lower_bound(written.begin(), written.end(), k);
        if (it != written.end() && *it == k) return false;
        written.insert(it, k);
        return true;
    };
    for (const PmAccess& a : init)
        for (int c = a.c0; c < a.c0 + a.nch; ++c)
            if (!put(a.res, a.dstep, c)) return 1;
    for (int tick = 0; tick < n_ticks; ++tick)
        for (int s = 0; s < n_slots; ++s) {
            for (const PmMeta& m : metas) {
                const int t = tick - m.lag;
                if (m.slot != s || t < 0 || t >= S) continue;
                for (const PmAccess& a : m.rd)
                    for (int c = a.c0; c < a.c0 + a.nch; ++c)
                        if (!has(a.res, t + a.dstep, c)) return 2;
            }
            for (const PmMeta& m : metas) {
                const int t = tick - m.lag;
                if (m.slot != s || t < 0 || t >= S) continue;
                for (const PmAccess& a : m.wr)
                    for (int c = a.c0; c < a.c0 + a.nch; ++c)
                        if (!put(a.res, t + a.dstep, c)) return 3;
            }
        }
    for (int t = 1; t <= S; ++t)
        if (!has(RES_X, t, 0)) return 4;
    return 0;
}

// ----------------------------------------------------------------------------- decoder (sampling)
// A decode descriptor as the planners see it: ParrotSampleDesc and, behind it, the forced frames of a ParrotSampleForcedDesc
// (all null: none).  parrot_sample_create and its kin plan the first, their _forced twins the second, through the same code.
struct SampleDescX : ParrotSampleDesc {
    const float* forced = nullptr;
    const int* n_forced = nullptr;
    float* own_x = nullptr;
    SampleDescX() : ParrotSampleDesc() {}
    SampleDescX(const ParrotSampleDesc& b) : ParrotSampleDesc(b) {}
    SampleDescX(const ParrotSampleForcedDesc& f) : ParrotSampleDesc(f.base), forced(f.forced), n_forced(f.n_forced), own_x(f.own_x) {}
};
struct SamplePlan : PlanBase {
    SampleDescX d;
    int esplit = 1;

    int enqueue(int, hipStream_t s) override {
        has_run = true;
        return live ? run_persist(s) : run_all(s);
    }

    // ---- per-row controls (parrot_sample_set_row_controls) --------------------------------------------------------------
    // Not part of the descriptor and not of pm_prog: a plan without them is, record for record, the plan it was.  With them
    // every consumer of d.timing / d.sharpening / d.sampling_bias reads element b of an array instead, on both paths; a
    // control the caller left null reads an array of the plan's own that holds the descriptor's scalar B times, so the
    // kernels have one flavour with the controls and one without.
    PmRows rows = {nullptr, nullptr, nullptr};
    bool has_rows = false, has_run = false;
    float* rows_own = nullptr;  // [3][B]: timing | sharpening | bias
    ~SamplePlan() override {
        if (rows_own) hipFree(rows_own);
    }
    int set_row_controls(const float* timing, const float* sharpening, const float* bias) {
        if (has_run) return PARROT_ERR_BADARG;  // a captured graph holds the pointers by value
        if (bias && d.gmm_K <= 0) return PARROT_ERR_BADARG;
        if (!timing && !sharpening && !bias) {
            has_rows = false;
            return 0;
        }
        const int rc = own_rows();
        if (rc != 0) return rc;
        rows.timing = timing ? timing : rows_own;
        rows.sharpening = sharpening ? sharpening : rows_own + d.B;
        rows.bias = bias ? bias : rows_own + (size_t)2 * d.B;
        has_rows = true;
        return 0;
    }

    // ---- persistent phase machine for the decode loop (persist.h) ------------------------------------------------
    // One resident kernel runs all S steps; a step = 2L + 3 phases: G_0, C_0, ATT, (G_l, C_l for l >= 1), readout,
    // output.  With output feedback (x_{t-1} -> layer inputs, model.py:899-924) the whole step is one dependency chain,
    // so every phase is on the critical path and costs its fixed latency (~4 us) instead of a launch (~16 us at
    // M = 16).  Each unit reads ONE fragment-major slab assembled by its producers:
    //   XG[l][t] / XC[l][t] = [h_l[t] or r*h_l ; w ; h_0[t+1] .. h_{l-1}[t+1] ; x[t] (64 columns, zero padded)]
    //   XR[t] = [h_0[t+1] .. h_{L-1}[t+1] ; w[t+1]]      XO[t] = readout[t]
    // Weights: fragment-major copies prepared by the caller (Wg_t / Wc_t: packed layer matrix with the feedback rows
    // appended and padded to 64; Wr_t; Wo_t with the columns padded to 64).
    enum Program { NONE, WHOLE, PIECES, PIECES_FBC, LSTM };
    Program program = NONE;  // what pm_prog holds: planned, replayed and placed (dry runs stop there)
    bool live = false;       // ... and uploaded: the launches go to the machine
    PmProgram pm_prog;
    PmSlabs sl;
    int pieces_info[16] = {0};
    unsigned long long plan_digest = 0;  // PmBuilder::digest of the program; 0: none

    // ---- forced frames (ParrotSampleForcedDesc::forced / n_forced / own_x; PmForce, persist.h) --------------------------------
    // A property of the plan: the unit that produces the fed-back frame selects between its own value and the forced one
    // (linear_tiles marks it; the sampling rows of a GMM head need no mark), so the frame must be ON the step's chain --
    // fbc_wanted refuses, and a GRU stack with an MSE head gets the 2L + 2 phases of PARROT_PM_FBC=0.  The attention fold does
    // not depend on the composed path (attfold_wanted; the candidate units of either cut carry it) and stays.  The kernels
    // with forcing always carry the row controls: a plan the caller gave none reads arrays of the descriptor's scalars.
    static bool forced(const SampleDescX& d) { return d.forced || d.n_forced || d.own_x; }
    PmForce force() const { return PmForce{d.forced, d.n_forced, d.own_x, d.B, d.O, d.ldx, 0}; }
    int own_rows() {
        if (rows_own) return 0;
        PH_CHECK(hipMalloc(reinterpret_cast<void**>(&rows_own), (size_t)3 * d.B * sizeof(float)));
        std::vector<float> host((size_t)3 * d.B);
        for (int b = 0; b < d.B; ++b) {
            host[b] = d.timing; host[(size_t)d.B + b] = d.sharpening; host[(size_t)2 * d.B + b] = d.sampling_bias;
        }
        PH_CHECK(hipMemcpy(rows_own, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }

    static bool persist_eligible_shape(const SampleDescX& d) {  // (no device query: the CPU tests plan too)
        if (d.bf16 && forced(d)) return false;  // (the kernels with forcing have no bf16 K loop: refused, parrot_sample_create)
        if (d.layer_norm || (d.gmm_K > 0 && !gmm_eligible(d)) || d.B > 64 || (d.H % 16) || (d.E % 16) || (d.R % 16) ||
            d.U > PM_ATT_MAXU || d.A > PM_ATT_MAXA || d.S < 1 || d.O > 64 || d.ldx < 64 || (d.ldx % 4))
            return false;
        if (d.bf16) return bf16_eligible(d);
        for (int l = 0; l < d.L; ++l)
            if (!d.Wg_t[l] || (d.cell == 0 && !d.Wc_t[l])) return false;
        return true;
    }
    // GMM head (ParrotSampleDesc::gmm_K > 0), opt-in through PARROT_PM_GMM=1 -- read HERE and nowhere else in the library:
    // the readout stack and the three head projections composed by the caller (Wrh_t / rh_const, rh_cols = NH16 columns) run
    // as NH16 / 16 plain LINEAR units into a write-once head history [S, B, NH16]; one PM_SAMPLE unit per batch row (persist.h)
    // then picks the component and writes x[t + 1].  The two whole-K programs take it (build_persist_whole,
    // build_persist_lstm); the step cut along K does not (sampling is not linear in h: no Wgx_t / Wcx_t, no attention fold).
    static bool gmm_eligible(const SampleDescX& d) {
        if (env_int("PARROT_PM_GMM", 0) == 0) return false;
        if (d.bf16 || d.gmm_K > 64 || !d.Wrh_t || !d.rh_const || (d.rh_cols % 16) || d.rh_cols < 2 * d.O * d.gmm_K + d.gmm_K) return false;
        return d.unif && d.noise && d.pi_out;
    }
    static int lstm_maxu(const SampleDescX& d, int nwg) { return std::max(d.H / 4, d.B) <= nwg ? 1 : 2; }
    // the head's column tiles need a place each in their phase (256 workgroups take K = 20: 159 tiles; 64 take K <= 8)
    static bool head_fits(const SampleDescX& d, int nwg) {
        return d.gmm_K <= 0 || d.rh_cols / 16 <= nwg * (d.cell == 1 ? lstm_maxu(d, nwg) : 1);
    }
    static long long head_floats(const SampleDescX& d) { return d.gmm_K > 0 ? (long long)d.S * d.B * d.rh_cols + 16 : 0; }
    // bf16 operands (ParrotSampleDesc::bf16): 32-deep K steps, the bf16 copies in place of Wg_t (GRU: and Wc_t).  LSTM
    // stacks; GRU stacks are opt-in through PARROT_PM_GRU_BF16=1 -- read HERE and nowhere else in the library -- with an MSE
    // head (a GMM head never qualifies under bf16: gmm_eligible; layer_norm never reaches this).  A descriptor that asks for
    // bf16 operands and does not qualify gets NO machine plan -- parrot_sample_create then refuses it.
    static bool bf16_eligible(const SampleDescX& d) {
        if ((d.cell != 0 && d.cell != 1) || (d.H % 32) || (d.E % 32)) return false;
        if (d.cell == 0 && (env_int("PARROT_PM_GRU_BF16", 0) == 0 || d.gmm_K > 0 || d.layer_norm)) return false;
        for (int l = 0; l < d.L; ++l)
            if (!d.Wg_t16[l] || (d.cell == 0 && !d.Wc_t16[l])) return false;
        return true;
    }
    // The weights of a product: fragment-major f32 blocks, or (w16) the bf16 copy in the machine's K order -- tile() below.
    struct PmW { const void* p; bool w16; };
    static PmW w32(const float* W) { return {W, false}; }
    // layer l's gate (kind 0) / candidate (kind 1) matrix of a GRU program
    PmW layer_w(int kind, int l) const {
        if (d.bf16) return {kind == 0 ? d.Wg_t16[l] : d.Wc_t16[l], true};
        return w32(kind == 0 ? d.Wg_t[l] : d.Wc_t[l]);
    }
    // LSTM stacks (cell == 1): one phase per layer, readout and output composed (Wro_t / ro_const) -- build_persist_lstm
    static bool lstm_eligible(const SampleDescX& d) {
        if (d.gmm_K > 0) return d.cell == 1 && d.L + 3 <= PM_MAXSLOTS;  // (persist_eligible_shape: Wrh_t / rh_const are there)
        return d.cell == 1 && d.Wro_t && d.ro_const && d.L + 2 <= PM_MAXSLOTS;
    }
    static bool whole_eligible(const SampleDescX& d) {  // GRU, whole-K phases -- build_persist_whole
        if (d.gmm_K > 0) return 2 * d.L + 3 <= PM_MAXSLOTS;  // (head and sampling phases in place of readout and output)
        if (2 * d.L + 3 > PM_MAXSLOTS || !d.Wr_t || !d.Wo_t || !d.bo_pad) return false;
        return (d.oadd != nullptr) == (d.oadd_pad != nullptr);
    }
    static bool persist_eligible(const SampleDescX& d) {
        if (!persist_eligible_shape(d)) return false;
        if (d.cell == 1 ? !lstm_eligible(d) : !(whole_eligible(d) || pieces_wanted(d))) return false;
        return pm_max_workgroups() >= 64 && head_fits(d, pm_max_workgroups());
    }
    static int fb_rows(const SampleDescX& d, int l) { return d.Wfg[l] ? 64 : 0; }
    static long long kslab(const SampleDescX& d, int l) { return d.H + d.E + (long long)l * d.H + fb_rows(d, l); }
    static long long persist_floats(const SampleDescX& d, int nwg) {
        const long long rows = pm_rows(d.B), S = d.S;
        if (d.cell == 1) {  // one slab per layer, the composed output's slab, h and c histories (build_persist_lstm)
            long long n = pm_header_floats((long long)(d.L + 2 + (d.gmm_K > 0 ? 1 : 0)) * nwg * 2);
            for (int l = 0; l < d.L; ++l) n += (S + 1) * rows * kslab(d, l);
            n += S * rows * ((long long)d.L * d.H + d.E);
            n += 2 * (long long)d.L * (S + 1) * d.B * d.H + S * d.B * d.A;
            return n + head_floats(d) + 4096;
        }
        long long n = pm_header_floats((long long)(2 * d.L + 3) * nwg);
        for (int l = 0; l < d.L; ++l) n += 2 * (S + 1) * rows * kslab(d, l);
        const long long ro = d.gmm_K > 0 ? 0 : d.R;  // (a GMM head has neither the readout's slab nor its history)
        n += S * rows * ((long long)d.L * d.H + d.E) + S * rows * ro;
        n += (long long)d.L * (S + 1) * d.B * d.H + (long long)d.L * S * d.B * d.H;   // h and z histories (row-major)
        n += S * d.B * ro + S * d.B * d.A;
        return n + piece_floats(d) + head_floats(d) + 4096;
    }
    // the bound of a planner's carve-up: the caller's workspace; dry runs carve what the size query asks for
    long long ws_limit(bool dry, int nwg) const { return dry ? persist_floats(d, nwg) : d.persist_ws_floats; }

    // The one planning entry: the program the descriptor and the switches ask for.  dry: plan, replay and place only, on
    // nwg_dry workgroups, no device memory is touched (parrot_sample_plan_pieces_dry / _digest_dry: the CPU tests plan every
    // program this way).
    void plan_persist(bool dry, int nwg_dry) {
        program = NONE;
        live = false;
        plan_digest = 0;
        if (!persist_eligible_shape(d)) return;  // (bf16 that does not qualify: no plan rather than an f32 one)
        const int nwg = dry ? nwg_dry : pm_max_workgroups();
        if (nwg < 64 || !head_fits(d, nwg)) return;
        if (!dry && (!d.persist_ws || d.persist_ws_floats < persist_floats(d, nwg))) return;
        if (d.cell == 1) {
            if (lstm_eligible(d)) build_persist_lstm(dry, nwg);
            return;
        }
        if (pieces_wanted(d)) build_persist_pieces(dry, nwg);                     // the step cut along K by the age of its operands
        if (program == NONE && whole_eligible(d)) build_persist_whole(dry, nwg);  // else the 2L + 3 whole-K phases
    }
    // How every planner ends: replay verdict in, placement, upload unless dry; which program the plan now holds.
    void finish(PmBuilder& pb, Program p, int n_ticks, int chk) {
        const bool ok = pb.finish(d.S, n_ticks, chk, pieces_info);
        plan_digest = pb.digest;
        program = ok ? p : NONE;
        live = ok && !pb.dry;
    }
    // End-of-utterance stop (ParrotSampleDesc::eou_extra > 0): a property of the launch, not of a program -- every program
    // above gets it the same way, through PmAtt (persist.h).  A descriptor that asks for it and does not qualify gets NO
    // machine plan, and parrot_sample_create then refuses it: the per-step launches cannot stop.
    static bool stop_eligible(const SampleDescX& d) {
        return d.eou_extra >= PM_EOU_MIN_EXTRA && d.eou_pos && d.eou_ncmp && d.eou_first;
    }
    bool stops_early() const { return live && pm_prog.att.eou_extra > 0; }
    int build_persist() {
        if (env_int("PARROT_SAMPLE_PERSIST", 1) == 0) return 0;
        if (!persist_eligible(d) || !d.persist_ws) return 0;
        if (d.eou_extra > 0 && !stop_eligible(d)) return 0;
        plan_persist(false, 0);
        if (live && d.eou_extra > 0) {
            PmAtt& a = pm_prog.att;
            a.eou_pos = d.eou_pos; a.eou_ncmp = d.eou_ncmp; a.eou_first = d.eou_first; a.eou_extra = d.eou_extra;
        }
        return 0;
    }

    // ---- what the three decode programs share: the carve-up, one emitter per unit kind, the tail -------------------------
    // The workspace in the order every program holds it (take() order = addresses): per layer the gate slab and, for a GRU,
    // the candidate slab; XR; with R_out the readout's slab; then the row-major histories.  extra0: K rows appended to
    // layer 0's slabs, behind the fed-back frame (the fbc program keeps the last layer's state there).
    void carve(PmBuilder& pb, long long extra0, int R_out) {
        const int L = d.L, S = d.S, B = d.B;
        const long long rows = pb.rows, BH = (long long)B * d.H;
        sl = PmSlabs();
        sl.L = L; sl.hc = d.H / 16; sl.ec = d.E / 16;
        for (int l = 0; l < L; ++l) {
            sl.kx[l] = kslab(d, l) + (l == 0 ? extra0 : 0);
            sl.fbch[l] = fb_rows(d, l) ? (int)(kslab(d, l) / 16) - 4 : -1;
            sl.XG[l] = pb.take((S + 1) * rows * sl.kx[l]);
            if (d.cell == 0) sl.XC[l] = pb.take((S + 1) * rows * sl.kx[l]);
        }
        sl.kr = (long long)L * d.H + d.E;
        sl.XR = pb.take(S * rows * sl.kr);
        if (R_out) sl.XO = pb.take(S * rows * R_out);
        pb.fm_end();
        for (int l = 0; l < L; ++l) sl.h[l] = pb.take((S + 1) * BH);
        for (int l = 0; l < L; ++l) {
            if (d.cell == 0) sl.z[l] = pb.take(S * BH);
            else sl.c[l] = pb.take((S + 1) * BH);
        }
        if (R_out) sl.ro_hist = pb.take((long long)S * B * R_out);
        sl.b_hist = pb.take((long long)S * B * d.A);
        if (d.gmm_K > 0) sl.head = pb.take((long long)S * B * d.rh_cols);
    }

    // Column tile ct of a product over `in`, W = its fragment-major weights ([N / 16][ks / 16] blocks of 16 x 16); `parts`
    // are added in the epilogue.  The meta of the kind starts the same way: what every tile of it reads.
    // W.w16: a PM_GEMM16 unit on the tile's bf16 slab, [N / 16][ks / 32] blocks of 1 KB (32 K-rows each), so the chunk range
    // must start and end on a 32-row boundary: every piece boundary does when H and E are multiples of 32 (the fed-back
    // rows are 64); a range that does not fails the build.
    PmReq tile(PmBuilder& pb, const PmIn& in, PmW W, int ct, const std::vector<PmPart>& parts, int N) const {
        PmReq q = pb.gemm(in.slot, in.slab, in.ks, in.c0, in.nch * 16, in.lag);
        if (W.w16) {
            if ((in.c0 & 1) || (in.nch & 1) || (in.ks % 32)) pb.failed = true;
            q.u.kind = PM_GEMM16;
            q.u.W = reinterpret_cast<const float*>(static_cast<const char*>(W.p) + ((size_t)ct * (in.ks / 32) + in.c0 / 2) * 1024);
        } else {
            q.u.W = static_cast<const float*>(W.p) + ((size_t)ct * (in.ks / 16) + in.c0) * 256;
        }
        for (const PmPart& p : parts) pb.add_operand(q.u, pm_rm(p.buf + 16 * ct, (long long)d.B * N, N));
        return q;
    }
    static PmMeta meta(const PmIn& in, const std::vector<PmPart>& parts) {
        PmMeta m;
        m.lag = in.lag; m.slot = in.slot;
        m.rd.push_back(pm_acc(in.res, 0, in.c0, in.nch));
        for (const PmPart& p : parts) m.rd.push_back(pm_acc(p.res, 0, 0, 1));
        return m;
    }
    // G_l: z -> its history, r * h_l[t] -> the head of the candidate slab
    void gate_tiles(PmBuilder& pb, std::vector<PmMeta>& metas, const PmIn& in, PmW W, int l, const std::vector<PmPart>& parts) {
        const int H = d.H;
        const long long BH = (long long)d.B * H;
        for (int ct = 0; ct < 2 * H / 16; ++ct) {
            PmReq q = tile(pb, in, W, ct, parts, 2 * H);
            PmUnit& u = q.u;
            u.bias = d.bg[l] ? d.bg[l] + 16 * ct : nullptr;
            if (d.seq_g[l]) pb.add_operand(u, pm_rm(d.seq_g[l] + 16 * ct, 0, 2 * H));
            u.epi = PM_EPI_GATES;
            u.rtile = 16 * ct >= H;
            if (!u.rtile) {
                u.o1 = pm_rm(sl.z[l] + 16 * ct, BH, H);
            } else {
                const int j0 = 16 * ct - H;
                u.e0 = pm_rm(sl.h[l] + j0, BH, H);
                pb.add_dst(u, pb.dst(sl.XC[l], 0, sl.kx[l], j0 / 16));
            }
            pb.push(q);
        }
        PmMeta m = meta(in, parts);
        m.rd.push_back(pm_acc(RES_H + l, 0, 0, 1));
        m.wr.push_back(pm_acc(RES_Z + l, 0, 0, 1));
        m.wr.push_back(pm_acc(RES_XC + l, 0, 0, sl.hc));
        metas.push_back(m);
    }
    // C_l -> h_l[t+1], into `tos`.  pp: this tile's share of the attention projection h_1 . Watt goes there (layer 0's
    // tiles of a program that folds it, PmUnit::pw / pp), else null.
    void cand_tiles(PmBuilder& pb, std::vector<PmMeta>& metas, const PmIn& in, PmW W, int l, const std::vector<PmPart>& parts,
                    const std::vector<PmTo>& tos, float* pp) {
        const int H = d.H, B = d.B, hc = sl.hc;
        const long long BH = (long long)B * H;
        for (int ct = 0; ct < hc; ++ct) {
            PmReq q = tile(pb, in, W, ct, parts, H);
            PmUnit& u = q.u;
            u.bias = d.bc[l] ? d.bc[l] + 16 * ct : nullptr;
            if (d.seq_c[l]) pb.add_operand(u, pm_rm(d.seq_c[l] + 16 * ct, 0, H));
            u.epi = PM_EPI_CAND;
            u.e0 = pm_rm(sl.h[l] + 16 * ct, BH, H);
            u.e1 = pm_rm(sl.z[l] + 16 * ct, BH, H);
            u.out = pm_rm(sl.h[l] + BH + 16 * ct, BH, H);
            add_tos(pb, u, tos, ct);
            if (pp) {
                u.pw[0] = d.Watt_t + (size_t)ct * 256;
                u.pw[1] = d.Watt_t + (size_t)(hc + ct) * 256;
                u.pp = pm_rm(pp + (size_t)ct * B * 32, (long long)hc * B * 32, 32);
            }
            pb.push(q);
        }
        PmMeta m = meta(in, parts);
        m.rd.push_back(pm_acc(RES_H + l, 0, 0, 1));
        m.rd.push_back(pm_acc(RES_Z + l, 0, 0, 1));
        m.wr.push_back(pm_acc(RES_H + l, 1, 0, 1));
        wr_tos(m, tos, hc);
        if (pp) m.wr.push_back(pm_acc(RES_PP, 0, 0, 1));
        metas.push_back(m);
    }
    // Every plain product -- a piece's partial sums, readout, output frame, x_pre, GMM head: the N / 16 column tiles of
    // in . W + bias + parts + add ([B, N] row-major, the same for every step) -> out (row-major, `wr` in the replay) and `tos`.
    // crit: on the step's dependency chain (pm_place serves those first).
    void linear_tiles(PmBuilder& pb, std::vector<PmMeta>& metas, const PmIn& in, PmW W, int N, const std::vector<PmPart>& parts,
                      const float* bias, const float* add, PmRM out, PmAccess wr, const std::vector<PmTo>& tos, bool crit = true) {
        for (int ct = 0; ct < N / 16; ++ct) {
            PmReq q = tile(pb, in, W, ct, parts, N);
            PmUnit& u = q.u;
            q.crit = crit ? 1 : 0;
            u.bias = bias ? bias + 16 * ct : nullptr;
            if (add) pb.add_operand(u, pm_rm(add + 16 * ct, 0, N));
            u.epi = PM_EPI_LINEAR;
            if (forced(d) && wr.res == RES_X) u.rtile = 1 + ct;  // the frame's unit of a forced plan does the select (PmForce)
            u.out = pm_rm(out.p + 16 * ct, out.st, out.ld);
            add_tos(pb, u, tos, ct);
            pb.push(q);
        }
        PmMeta m = meta(in, parts);
        m.wr.push_back(wr);
        wr_tos(m, tos, N / 16);
        metas.push_back(m);
    }
    PmRM x_next() const { return pm_rm(d.x + (size_t)d.B * d.ldx, (long long)d.B * d.ldx, d.ldx); }  // x[t+1] (63 columns, padded to 64)
    // The attention: one unit per batch row; with_pp: it reads the projection's partial sums of cand_tiles
    void att_rows(PmBuilder& pb, std::vector<PmMeta>& metas, int slot, int lag, bool with_pp) {
        pb.att_rows(slot, lag);
        PmMeta m;
        m.lag = lag; m.slot = slot;
        m.rd.push_back(pm_acc(RES_H, 1, 0, 1));
        if (with_pp) m.rd.push_back(pm_acc(RES_PP, 0, 0, 1));
        m.rd.push_back(pm_acc(RES_KAPPA, 0, 0, 1));
        m.wr.push_back(pm_acc(RES_KAPPA, 1, 0, 1));
        wr_tos(m, sl.w_tos(), sl.ec);
        metas.push_back(m);
    }
    // GMM head, both whole-K programs: the composed head's column tiles XR . Wrh_t + rh_const -> head history (row-major,
    // write-once, no fragment-major copies) in phase `slot`, then one sampling unit per batch row: head history -> x[t+1]
    // and the fed-back chunks; and what the sampling rows read (PmSamp)
    void head_phases(PmBuilder& pb, std::vector<PmMeta>& metas, int slot) {
        const int NH = d.rh_cols;
        linear_tiles(pb, metas, {slot, 0, sl.XR, sl.kr, RES_XR, 0, (int)(sl.kr / 16)}, w32(d.Wrh_t), NH, {}, nullptr, d.rh_const,
                     pm_rm(sl.head, (long long)d.B * NH, NH), pm_acc(RES_HEAD, 0, 0, 1), {});
        const std::vector<PmTo> tos = sl.frame_tos();
        std::vector<PmDst> fb;
        for (const PmTo& t : tos) fb.push_back(pb.dst(t.slab, t.dstep, t.ks, t.c0));
        pb.sample_rows(slot + 1, 0, fb);
        PmMeta m;
        m.lag = 0; m.slot = slot + 1;
        m.rd.push_back(pm_acc(RES_HEAD, 0, 0, 1));
        m.wr.push_back(pm_acc(RES_X, 1, 0, 1));
        wr_tos(m, tos, 4);
        metas.push_back(m);
    }
    void samp_common(float* head) {
        PmSamp& sp = pm_prog.samp;
        sp.head = pm_rm(head, (long long)d.B * d.rh_cols, d.rh_cols);
        sp.unif = d.unif; sp.noise = d.noise; sp.pi = d.pi_out;
        sp.x = d.x + (size_t)d.B * d.ldx;
        sp.B = d.B; sp.O = d.O; sp.K = d.gmm_K; sp.ldx = d.ldx;
        sp.bias = d.sampling_bias; sp.eps = d.eps;
    }
    // What every program ends with: the attention's and the sampling's records, the entering states converted into slot 0
    // of the slabs, the buffers that start EMPTY in dataflow mode.  Returns the same entering states for the replay.
    std::vector<PmAccess> tail(PmBuilder& pb) {
        const int H = d.H, E = d.E, L = d.L, hc = sl.hc;
        const long long SBH = (long long)d.S * d.B * H, BH = (long long)d.B * H;
        std::vector<PmAccess> init;
        pb.att_common(d, sl.h[0]);
        pm_prog.att.b = sl.b_hist;
        if (sl.head) samp_common(sl.head);
        for (const PmTo& t : sl.w_tos()) pb.add_wdst(pb.dst(t.slab, t.dstep, t.ks, t.c0));
        for (int l = 0; l < L; ++l) {  // initial states (slot 0 of the ping-pong)
            pb.add_init(d.h[l], H, H, sl.XG[l], sl.kx[l], 0);
            init.push_back(pm_acc(RES_XG + l, 0, 0, hc));
            init.push_back(pm_acc(RES_H + l, 0, 0, 1));
            if (sl.c[l]) init.push_back(pm_acc(RES_C + l, 0, 0, 1));
        }
        sl.each_slab(0, [&](const float* s, int res) {
            pb.add_init(d.w, E, E, s, sl.kx[0], hc);
            init.push_back(pm_acc(res, 0, hc, sl.ec));
        });
        init.push_back(pm_acc(RES_KAPPA, 0, 0, 1));
        // x[0] = 0 (model.py:834-835): slot 0 of d.x, converted like the other entering states (the slabs start EMPTY in
        // dataflow mode, so "stays at the zero fill" is not enough)
        for (int l = 0; l < L; ++l)
            if (sl.fbch[l] >= 0)
                sl.each_slab(l, [&](const float* s, int res) {
                    pb.add_init(d.x, d.ldx, 64, s, sl.kx[l], sl.fbch[l]);
                    init.push_back(pm_acc(res, 0, sl.fbch[l], 4));
                });
        pb.fill_fm();
        for (int l = 0; l < L; ++l) {
            pb.add_fill(sl.h[l] + BH, SBH);
            if (sl.z[l]) pb.add_fill(sl.z[l], SBH);
            if (sl.c[l]) pb.add_fill(sl.c[l] + BH, SBH);
        }
        if (sl.head) pb.add_fill(sl.head, (long long)d.S * d.B * d.rh_cols);
        return init;
    }

    // ---- GRU, whole-K phases: every product walks its whole slab, nothing lags ------------------------------------------
    static int slotG(int l) { return l == 0 ? 0 : 2 * l + 1; }
    static int slotC(int l) { return slotG(l) + 1; }
    void build_persist_whole(bool dry, int nwg) {
        const int B = d.B, L = d.L, R = d.R, n_slots = 2 * L + 3;
        const bool gmm = d.gmm_K > 0;  // readout and output phases -> composed head and sampling phases
        PmBuilder pb(pm_prog, dry, d.persist_ws, ws_limit(dry, nwg), B, nwg, n_slots, 1);
        carve(pb, 0, gmm ? 0 : R);
        if (pb.failed) return;
        std::vector<PmMeta> metas;
        for (int l = 0; l < L; ++l) {
            const int nch = (int)(sl.kx[l] / 16);
            gate_tiles(pb, metas, {slotG(l), 0, sl.XG[l], sl.kx[l], RES_XG + l, 0, nch}, layer_w(0, l), l, {});
            cand_tiles(pb, metas, {slotC(l), 0, sl.XC[l], sl.kx[l], RES_XC + l, 0, nch}, layer_w(1, l), l, {}, sl.state_tos(l), nullptr);
        }
        att_rows(pb, metas, 2, 0, false);
        if (gmm) {
            head_phases(pb, metas, 2 * L + 1);
        } else {
            linear_tiles(pb, metas, {2 * L + 1, 0, sl.XR, sl.kr, RES_XR, 0, (int)(sl.kr / 16)}, w32(d.Wr_t), R, {}, d.br, d.radd,
                         pm_rm(sl.ro_hist, (long long)B * R, R), pm_acc(RES_RO, 0, 0, 1), {{sl.XO, R, RES_XO, 0, 0}});
            linear_tiles(pb, metas, {2 * L + 2, 0, sl.XO, R, RES_XO, 0, R / 16}, w32(d.Wo_t), 64, {}, d.bo_pad, d.oadd_pad, x_next(),
                         pm_acc(RES_X, 1, 0, 1), sl.frame_tos());
        }
        const std::vector<PmAccess> init = tail(pb);
        pm_prog.w16 = d.bf16 ? 1 : 0;  // (the layer units are PM_GEMM16; readout and output tiles stay f32 units)
        pm_prog.dataflow = sw_pm_dataflow(0);  // (measured no gain without barriers: 57.6 us per step either way at configs[2])
        memset(pieces_info, 0, sizeof(pieces_info));
        finish(pb, WHOLE, d.S, check_pieces(metas, init, n_slots, 4, 4));
    }
    int persist_status() const { return live ? pm_status(pm_prog) : 0; }
    int steps_run(int* steps) const {
        if (live) return pm_steps_run(pm_prog, steps);
        if (!steps) return PH_ERR_BADARG;
        PH_CHECK(hipDeviceSynchronize());
        *steps = d.S;
        return 0;
    }

    // ---- decode state out and in (parrot_sample_save_state / _load_state; the kernels: decode_state.hip) -------------------
    // What a row carries from frame t to frame t + 1, packed [B, W]: x, kappa, w, the layers' states, an LSTM's cells.  Every
    // path ENTERS through slot 0 of d.x / d.kappa / d.w / d.h[l] / d.cwork[l] (tail(): the init records; run_persist; run_all),
    // so loading is one scatter into them.  After frame S the first three lie in slot S of their histories; states and cells
    // in row S of the machine's histories (sl.h / sl.c), on the launches in the ping-pong slot the run ended on (S & 1).
    // at_entry: a state was loaded and no run has followed -- then THE state of the plan is the one in the entering slots.
    bool at_entry = false;
    int run(int which, hipStream_t s) override {
        at_entry = false;
        return PlanBase::run(which, s);
    }
    static long long state_floats(const ParrotSampleDesc& d) {
        return (long long)d.ldx + d.A + d.E + (long long)d.L * d.H * (d.cell == 1 ? 2 : 1);
    }
    DecodeStateSegs state_segs(bool entry) const {
        static_assert(3 + 2 * PARROT_MAX_LAYERS <= DECODE_STATE_MAXSEG, "a decode state has more pieces than DecodeStateSegs holds");
        const size_t t = entry ? 0 : (size_t)d.S, BH = (size_t)d.B * d.H;
        DecodeStateSegs s;
        s.B = d.B;
        s.add(d.x + t * d.B * d.ldx, d.ldx);
        s.add(d.kappa + t * d.B * d.A, d.A);
        s.add(d.w + t * d.B * d.E, d.E);
        for (int l = 0; l < d.L; ++l) s.add(entry ? d.h[l] : live ? sl.h[l] + t * BH : d.h[l] + (d.S & 1) * BH, d.H);
        for (int l = 0; l < d.L && d.cell == 1; ++l)
            s.add(entry ? d.cwork[l] : live ? sl.c[l] + t * BH : d.cwork[l] + (d.S & 1) * BH, d.H);
        return s;
    }
    int save_state(float* state, hipStream_t st) const {
        if (!state) return PARROT_ERR_BADARG;
        if (d.eou_extra > 0) return PARROT_ERR_UNSUPPORTED;  // a run that stopped early need not have a frame S
        if (!has_run && !at_entry) return PARROT_ERR_BADARG;  // neither a run nor a load: there is no state yet
        return decode_state_gather_launch(state_segs(at_entry), state, st);
    }
    int load_state(const float* state, hipStream_t st) {
        if (!state) return PARROT_ERR_BADARG;
        const int rc = decode_state_scatter_launch(state_segs(true), state, st);
        at_entry = at_entry || rc == 0;
        return rc;
    }

    int run_persist(hipStream_t st) {
        const size_t BH = (size_t)d.B * d.H;
        for (int l = 0; l < d.L; ++l) {  // row-major initial state for the epilogues (r * h_prev, state blend; LSTM: cells)
            PL_TRY((int)hipMemcpyAsync(sl.h[l], d.h[l], BH * sizeof(float), hipMemcpyDeviceToDevice, st));
            if (sl.c[l]) PL_TRY((int)hipMemcpyAsync(sl.c[l], d.cwork[l], BH * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        if (forced(d)) {  // (parrot_sample_create made rows_own for a forced plan)
            const PmRows own = {rows_own, rows_own + d.B, rows_own + (size_t)2 * d.B};
            return pm_launch_forced(pm_prog, st, has_rows ? rows : own, force());
        }
        return pm_launch(pm_prog, st, has_rows ? &rows : nullptr);
    }

    // ---- LSTM stacks on the machine ----------------------------------------------------------------------------------
    // An LSTM layer is ONE product [h_l[t] ; w ; h_0[t+1] .. h_{l-1}[t+1] ; x[t]] . W over the gate-interleaved columns
    // (sk_col order, Wg_t[l] = parrot_tile_weights(.., lstm_H = H)) with the cell update in the epilogue (PM_EPI_LSTM,
    // persist.hip), so a step is L + 2 dependent phases: layer 0, attention, layers 1 .. L-1, composed output
    // (x = XR . Wro + ro_const, as in the pieces plan).  Every product walks its whole K.  A layer has H / 4 tiles of 16
    // columns; each yields four state columns = a quarter of a fragment-major block (PmUnit::rtile), four neighbouring
    // units complete a block.  More tiles than workgroups (384 at H = 1536): two units per workgroup and phase (maxu 2).
    // The cell history [S + 1, B, H] is row-major and write-once like the state history (dataflow mode polls it).
    // ParrotSampleDesc::bf16: the layer units become PM_GEMM16 (persist.h) on the bf16 copies Wg_t16 -- the same slabs,
    // phases, epilogues and workspace; only the weight pointer, the unit kind and what pm_place charges for LDS differ.
    // The output tiles stay f32 units of the same program.
    static int slotL(int l) { return l == 0 ? 0 : l + 1; }
    void build_persist_lstm(bool dry, int nwg) {
        const int H = d.H, B = d.B, L = d.L, hc = H / 16;
        for (int l = 0; l < L && !dry; ++l)
            if (!d.cwork[l]) return;
        const long long BH = (long long)B * H;
        const bool gmm = d.gmm_K > 0;  // composed head phase + sampling phase in place of the composed output phase
        const int n_slots = L + 2 + (gmm ? 1 : 0), sATT = 1, sOUT = L + 1;
        const int maxu = lstm_maxu(d, nwg);
        const bool w16 = d.bf16 != 0;  // (persist_eligible_shape: the widths and the copies qualify)
        if (std::max(H / 4, B) > nwg * maxu || n_slots * maxu > PM_MAXENT) return;
        PmBuilder pb(pm_prog, dry, d.persist_ws, ws_limit(dry, nwg), B, nwg, n_slots, maxu);
        carve(pb, 0, 0);
        if (pb.failed) return;

        std::vector<PmMeta> metas;
        for (int l = 0; l < L; ++l) {
            const int nch = (int)(sl.kx[l] / 16);
            const std::vector<PmTo> tos = sl.state_tos(l);
            PmMeta m;
            m.lag = 0; m.slot = slotL(l);
            m.rd.push_back(pm_acc(RES_XG + l, 0, 0, nch));
            m.rd.push_back(pm_acc(RES_C + l, 0, 0, 1));
            m.wr.push_back(pm_acc(RES_C + l, 1, 0, 1));
            m.wr.push_back(pm_acc(RES_H + l, 1, 0, 1));
            wr_tos(m, tos, hc);
            metas.push_back(m);
            for (int ct = 0; ct < H / 4; ++ct) {
                PmReq q = pb.gemm(slotL(l), sl.XG[l], sl.kx[l]);
                PmUnit& u = q.u;
                if (w16) {  // the tile's bf16 slab: kx / 32 blocks of 1 KB (parrot_tile_weights_bf16, mode 2)
                    u.kind = PM_GEMM16;
                    u.W = reinterpret_cast<const float*>(static_cast<const char*>(d.Wg_t16[l]) + (size_t)ct * (nch / 2) * 1024);
                } else {
                    u.W = d.Wg_t[l] + (size_t)ct * nch * 256;
                }
                u.bias = d.bg[l] ? d.bg[l] + 4 * ct : nullptr;
                if (d.seq_g[l]) pb.add_operand(u, pm_rm(d.seq_g[l] + 4 * ct, 0, 4 * H));
                u.epi = PM_EPI_LSTM; u.gstr = H; u.rtile = ct & 3;
                u.e1 = pm_rm(sl.c[l] + 4 * ct, BH, H);
                u.o1 = pm_rm(sl.c[l] + BH + 4 * ct, BH, H);
                u.out = pm_rm(sl.h[l] + BH + 4 * ct, BH, H);
                add_tos(pb, u, tos, ct / 4);
                pb.push(q);
            }
        }
        att_rows(pb, metas, sATT, 0, false);
        if (gmm)
            head_phases(pb, metas, sOUT);
        else
            linear_tiles(pb, metas, {sOUT, 0, sl.XR, sl.kr, RES_XR, 0, (int)(sl.kr / 16)}, w32(d.Wro_t), 64, {}, nullptr, d.ro_const, x_next(),
                         pm_acc(RES_X, 1, 0, 1), sl.frame_tos());
        const std::vector<PmAccess> init = tail(pb);
        pm_prog.lstm = 1;
        pm_prog.w16 = w16 ? 1 : 0;
        // no grid barriers with one unit per workgroup and phase (34.9 against 38.7 us per step at 2 x 1024, B 16); with two
        // (H = 1536: 384 tiles on 256 workgroups, all weights streamed) the barriers measured faster: 114.8 against 124.9
        pm_prog.dataflow = sw_pm_dataflow(maxu == 1 ? 1 : 0);
        memset(pieces_info, 0, sizeof(pieces_info));
        pieces_info[13] = maxu;
        finish(pb, LSTM, d.S, check_pieces(metas, init, n_slots, 4, 4));
    }

    // ---- round 4: the decode step cut along K by the AGE of its operands ------------------------------------------
    // With the output fed back (model.py:899-924) a step is one dependency chain x[t] -> G_0 -> C_0 -> attention ->
    // G_1 -> C_1 .. -> readout -> output -> x[t+1], and above every phase walked the whole K of its product (1600 ..
    // 2624 rows at configs[2]) although only ONE operand of each product is new when the phase starts.  Here
    //   * readout and output are one phase: without GMM head and layer norm, x = (XR . Wr + br + radd) . Wo + bo + oadd is
    //     linear in XR (model.py:992-1013), so the caller hands over Wro = Wr . Wo ([L H + E, 64], fragment-major) and
    //     ro_const = (br + radd) . Wo + bo + oadd ([B, 64]); the readout itself is not an output of sample_model;
    //   * every product is cut into pieces along K, one per operand ([h_l ; w ; h_0 .. h_{l-1} ; x] are chunk ranges of
    //     the unit's slab).  The piece whose operand is produced by the phase just before the product's own is the
    //     CRITICAL unit (K = 64 for G_0, E for G_1, H for the candidates and the output); every other piece runs as a
    //     LINEAR unit on workgroups that are idle anyway (the decode loop keeps < 130 of 256 busy per phase), in a phase
    //     between its operand's and the product's, and leaves its [B, N] partial sums row-major and write-through; the
    //     critical unit adds them in its epilogue (PmUnit::add, up to 4).
    // A tick has 2L + 2 phases; main units run step (tick - 1), pieces whose operand dates from the previous step may run
    // in the previous tick (lag 0), so the launch has S + 1 ticks.  check_pieces() replays the table symbolically (every
    // read satisfied by a write of a strictly earlier phase, every buffer element written once) before it is used.
    // Round 5: the attention projection folded into layer 0's candidate units (PmUnit::pw / pp, persist.hip)
    static bool attfold_wanted(const SampleDescX& d) {
        // (bf16 operands: not taken -- the oracle's projection is an exact product of h_1, and the f32-only fold of
        // pm_gemm is not part of a PM_GEMM16 unit)
        return !d.bf16 && d.Watt_t && d.B <= 16 && 3 * d.A <= 32 && env_int("PARROT_PM_ATTFOLD", 1) != 0;
    }
    // Round 5 ("fbc"): the fed-back frame out of the chain.  x[t+1] = x_pre + h_{L-1}[t+1] . A (A = the last layer's rows of
    // Wr . Wo), so layer 0's next gates need  x_pre . Wfg  (x_pre is complete two phases before h_{L-1}) and
    // h_{L-1} . (A . Wfg)  -- the caller composes A . Wfg / A . Wfc and appends them to layer 0's matrices (Wgx_t / Wcx_t).
    // The output product then feeds nothing inside the loop: it runs beside the next step's gate phase, and a step is
    // 2L + 1 dependent phases (G_0 with K = H critical instead of K = 64, but one phase of ~5 us less).
    static bool fbc_wanted(const SampleDescX& d) {
        if (env_int("PARROT_PM_FBC", 1) == 0) return false;
        if (forced(d)) return false;  // x[t+1] = x_pre + h_{L-1} . A does not hold on a forced step: the frame stays on the chain
        if (d.bf16) return false;  // composed rows A . Wf would round at other points than the oracle's x . Wf
        if (d.L < 2 || !d.Wgx_t[0] || !d.Wcx_t[0] || !fb_rows(d, 0)) return false;
        for (int l = 1; l < d.L; ++l)
            if (fb_rows(d, l)) return false;
        return 2 * d.L + 1 <= PM_MAXSLOTS;
    }
    static long long kslab_p(const SampleDescX& d, int l, bool fbc) { return kslab(d, l) + ((fbc && l == 0) ? d.H : 0); }
    static int n_phases(const SampleDescX& d, bool fbc) { return fbc ? 2 * d.L + 1 : 2 * d.L + 2; }
    static int slot_pre(const SampleDescX& d) { return std::max(slotC(d.L - 2), 2) + 1; }  // (fbc) after x_pre's last operand
    static bool pieces_wanted(const SampleDescX& d) {
        return d.gmm_K <= 0 && d.Wro_t && d.ro_const && env_int("PARROT_PM_PIECES", 1) != 0 && 2 * d.L + 2 <= PM_MAXSLOTS;
    }
    static bool piece_groups(const SampleDescX& d, std::vector<PmGroup>& gs, bool fbc) {
        const int H = d.H, E = d.E, L = d.L, n = n_phases(d, fbc), sATT = 2, sOUT = fbc ? 0 : 2 * L + 1;
        const int hc = H / 16, ec = E / 16;
        auto pos = [&](int delta, int slot) { return (1 + delta) * n + slot; };
        auto piece = [](int c0, int nch, int gp) { PmPiece p; p.c0 = c0; p.nch = nch; p.gp = gp; p.crit = false; p.lag = 1; p.slot = -1; p.pbuf = -1; return p; };
        gs.clear();
        for (int l = 0; l < L; ++l)
            for (int kind = 0; kind < 2; ++kind) {
                PmGroup g;
                g.kind = kind; g.l = l; g.slot = kind == 0 ? slotG(l) : slotC(l); g.N = kind == 0 ? 2 * H : H; g.glag = 0;
                g.ks = kslab_p(d, l, fbc); g.res = (kind == 0 ? RES_XG : RES_XC) + l;
                g.pc.push_back(piece(0, hc, kind == 0 ? pos(-1, slotC(l)) : pos(0, slotG(l))));  // h_l[t] | r * h_l[t]
                g.pc.push_back(piece(hc, ec, l == 0 ? pos(-1, sATT) : pos(0, sATT)));              // w[t] | w[t+1]
                for (int j = 0; j < l; ++j) g.pc.push_back(piece(hc + ec + j * hc, hc, pos(0, slotC(j))));  // h_j[t+1]
                if (fb_rows(d, l) && !fbc) g.pc.push_back(piece((int)(g.ks / 16) - 4, 4, pos(-1, sOUT)));  // x[t]
                if (fb_rows(d, l) && fbc) {  // (l == 0) x_pre of the previous step, and the last layer's state . (A . Wf)
                    g.pc.push_back(piece(hc + ec, 4, pos(-1, slot_pre(d))));
                    g.pc.push_back(piece(hc + ec + 4, hc, pos(-1, slotC(L - 1))));
                }
                gs.push_back(g);
            }
        {
            PmGroup o;
            o.kind = 2; o.l = 0; o.slot = sOUT; o.N = 64; o.ks = (long long)L * H + E; o.res = RES_XR; o.glag = fbc ? 1 : 0;
            if (!fbc) {
                for (int j = 0; j < L; ++j) o.pc.push_back(piece(j * hc, hc, pos(0, slotC(j))));
                o.pc.push_back(piece(L * hc, ec, pos(0, sATT)));
            } else {  // x = x_pre (added in the epilogue) + h_{L-1} . A, beside the NEXT step's gate phase
                o.pc.push_back(piece((L - 1) * hc, hc, pos(0, slotC(L - 1))));
            }
            gs.push_back(o);
        }
        if (fbc) {
            PmGroup o;
            o.kind = 3; o.l = 0; o.slot = slot_pre(d); o.N = 64; o.ks = (long long)L * H + E; o.res = RES_XR; o.glag = 0;
            for (int j = 0; j + 1 < L; ++j) o.pc.push_back(piece(j * hc, hc, pos(0, slotC(j))));
            o.pc.push_back(piece(L * hc, ec, pos(0, sATT)));
            gs.push_back(o);
        }
        for (PmGroup& g : gs) {
            size_t ci = 0;
            for (size_t i = 1; i < g.pc.size(); ++i)
                if (g.pc[i].gp > g.pc[ci].gp) ci = i;
            if (g.pc[ci].gp >= (1 + g.glag) * n + g.slot) return false;
            g.pc[ci].crit = true;
            g.pc[ci].slot = g.slot;
            g.pc[ci].lag = 1 + g.glag;
            const int fixed = g.kind >= 2 ? 1 : ((g.kind == 0 ? d.seq_g[g.l] : d.seq_c[g.l]) ? 1 : 0);
            while ((int)g.pc.size() - 1 + fixed > 4) {  // more partial sums than a unit can add: join neighbours
                int best = -1, bestd = 1 << 30;
                for (size_t i = 0; i + 1 < g.pc.size(); ++i) {
                    const PmPiece &a = g.pc[i], &b = g.pc[i + 1];
                    if (a.crit || b.crit || a.c0 + a.nch != b.c0) continue;
                    const int dd = a.gp > b.gp ? a.gp - b.gp : b.gp - a.gp;
                    if (dd < bestd) { bestd = dd; best = (int)i; }
                }
                if (best < 0) return false;
                g.pc[best].nch += g.pc[best + 1].nch;
                g.pc[best].gp = std::max(g.pc[best].gp, g.pc[best + 1].gp);
                g.pc.erase(g.pc.begin() + best + 1);
            }
        }
        return true;
    }
    // the phase of every non-critical piece: most constrained first; a phase may not take more units than workgroups, and
    // a piece should not outlast the critical units of its phase (unit cost as in pm_place)
    static bool piece_slots(const SampleDescX& d, std::vector<PmGroup>& gs, int nwg, bool fbc) {
        const int n = n_phases(d, fbc);
        auto cost = [](int K) { return 3.5 + 3.5 * K / 1024.0; };
        std::vector<int> cnt(n, 0);
        std::vector<double> tcrit(n, 0.0);
        cnt[2] = d.B; tcrit[2] = 9.0;
        struct Ref { int g, p, ncand, K, tiles; };
        std::vector<Ref> refs;
        for (size_t gi = 0; gi < gs.size(); ++gi)
            for (size_t pi = 0; pi < gs[gi].pc.size(); ++pi) {
                PmGroup& g = gs[gi];
                PmPiece& p = g.pc[pi];
                if (p.crit) {
                    cnt[g.slot] += g.N / 16;
                    tcrit[g.slot] = std::max(tcrit[g.slot], cost(p.nch * 16));
                } else {
                    refs.push_back({(int)gi, (int)pi, (1 + g.glag) * n + g.slot - 1 - p.gp, p.nch * 16, g.N / 16});
                }
            }
        for (int s = 0; s < n; ++s)
            if (cnt[s] > nwg) return false;
        std::stable_sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) {
            if (a.ncand != b.ncand) return a.ncand < b.ncand;
            if (a.K != b.K) return a.K > b.K;
            return a.tiles > b.tiles;
        });
        for (const Ref& r : refs) {
            PmGroup& g = gs[r.g];
            PmPiece& p = g.pc[r.p];
            int best = -1;
            double best_score = 0;
            for (int q = p.gp + 1; q < (1 + g.glag) * n + g.slot; ++q) {
                const int s = q % n;
                if (cnt[s] + r.tiles > nwg) continue;
                const double late = cost(r.K) - tcrit[s];
                const double score = (late > 0 ? late : 0) * 1e3 + cnt[s] + r.tiles;
                if (best < 0 || score < best_score) { best = q; best_score = score; }
            }
            if (best < 0) return false;
            p.slot = best % n;
            p.lag = best / n;
            cnt[p.slot] += r.tiles;
        }
        return true;
    }
    // Joins the two neighbouring non-critical pieces (same product, adjacent chunk ranges) whose operands appear closest in
    // time -- ties: the widest product first, it frees the most units -- into one piece that waits for the later operand.
    // The plan with the fed-back frame out of the chain has one phase less to spread its pieces over (round 5).
    static bool join_closest_pieces(std::vector<PmGroup>& gs) {
        int bg = -1, bi = -1, bd = 1 << 30, bn = 0;
        for (size_t gi = 0; gi < gs.size(); ++gi) {
            const PmGroup& g = gs[gi];
            for (size_t i = 0; i + 1 < g.pc.size(); ++i) {
                const PmPiece &a = g.pc[i], &b = g.pc[i + 1];
                if (a.crit || b.crit || a.c0 + a.nch != b.c0) continue;
                const int dd = a.gp > b.gp ? a.gp - b.gp : b.gp - a.gp;
                if (dd < bd || (dd == bd && g.N > bn)) { bd = dd; bn = g.N; bg = (int)gi; bi = (int)i; }
            }
        }
        if (bg < 0) return false;
        PmGroup& g = gs[bg];
        g.pc[bi].nch += g.pc[bi + 1].nch;
        g.pc[bi].gp = std::max(g.pc[bi].gp, g.pc[bi + 1].gp);
        g.pc.erase(g.pc.begin() + bi + 1);
        return true;
    }
    static long long piece_floats(const SampleDescX& d) {  // the partial-sum buffers of the pieces (an upper bound:
        std::vector<PmGroup> gs;                                 // before any capacity-driven joins)
        const bool fbc = fbc_wanted(d);
        if (!pieces_wanted(d) || !piece_groups(d, gs, fbc)) return 0;
        long long n = 0;
        for (const PmGroup& g : gs)
            for (const PmPiece& p : g.pc)
                if (!p.crit) n += (long long)(d.S + 1) * d.B * g.N + 16;
        if (fbc) {  // the longer layer-0 slabs, x_pre row-major, the zero rows behind x[0]
            const long long rows = pm_rows(d.B);
            n += 2 * (long long)(d.S + 1) * rows * d.H + (long long)(d.S + 2) * d.B * 64 + (long long)d.B * d.H + 64;
        }
        if (attfold_wanted(d)) n += (long long)d.S * (d.H / 16) * d.B * 32 + 64;  // the projection's partial sums
        return n;
    }

    void build_persist_pieces(bool dry, int nwg) {
        std::vector<PmGroup> gs;
        const bool fbc = fbc_wanted(d);
        if (!piece_groups(d, gs, fbc)) return;
        while (!piece_slots(d, gs, nwg, fbc))   // more units than one per workgroup and phase: join two pieces and try again
            if (!join_closest_pieces(gs)) return;
        const int H = d.H, B = d.B, L = d.L, S = d.S;
        const int n_slots = n_phases(d, fbc), hc = H / 16;
        PmBuilder pb(pm_prog, dry, d.persist_ws, ws_limit(dry, nwg), B, nwg, n_slots, 1);
        carve(pb, fbc ? H : 0, 0);  // (fbc) layer 0's slabs: x_pre in the frame's chunks, then the last layer's state
        const int fbh = sl.fbch[0] + 4;
        const bool attfold = attfold_wanted(d) && pb.MB == 1;
        float* pp = attfold ? pb.take((long long)S * hc * B * 32) : nullptr;  // [S][H / 16][B][32] partial projections
        float* zero_rows = fbc ? pb.take((long long)B * H) : nullptr;            // never written: the workspace arrives zero-filled
        float* xpre_rm = fbc ? pb.take((long long)(S + 1) * B * 64) : nullptr;  // x_pre of step t, row-major (the output unit adds it)
        float* const part_base = pb.mark();
        int npart = 0;
        std::vector<float*> pbuf;
        for (PmGroup& g : gs)
            for (PmPiece& p : g.pc)
                if (!p.crit) {
                    p.pbuf = npart++;
                    pbuf.push_back(pb.take((long long)(S + 1) * B * g.N + 16));
                }
        float* const part_end = pb.mark();
        if (pb.failed) return;

        std::vector<PmMeta> metas;
        for (const PmGroup& g : gs) {
            const int l = g.l, N = g.N;
            const float* slab = g.kind == 0 ? sl.XG[l] : (g.kind == 1 ? sl.XC[l] : sl.XR);
            // (bf16 operands: the layer products on the bf16 copies, never composed -- fbc_wanted; the output tiles stay f32)
            const PmW Wt = g.kind >= 2 ? w32(d.Wro_t)
                                       : ((fbc && l == 0) ? w32(g.kind == 0 ? d.Wgx_t[0] : d.Wcx_t[0]) : layer_w(g.kind, l));
            std::vector<PmPart> parts;  // what the critical unit adds: the other pieces' sums
            for (const PmPiece& o : g.pc)
                if (!o.crit) parts.push_back({pbuf[o.pbuf], RES_PART + o.pbuf});
            for (const PmPiece& p : g.pc) {
                const PmIn in = {p.slot, p.lag, slab, g.ks, g.res, p.c0, p.nch};
                if (!p.crit) {
                    linear_tiles(pb, metas, in, Wt, N, {}, nullptr, nullptr, pm_rm(pbuf[p.pbuf], (long long)B * N, N),
                                 pm_acc(RES_PART + p.pbuf, 0, 0, 1), {}, false);
                } else if (g.kind == 0) {
                    gate_tiles(pb, metas, in, Wt, l, parts);
                } else if (g.kind == 1) {
                    std::vector<PmTo> tos = sl.state_tos(l);
                    if (fbc && l == L - 1)  // ... and the operand of layer 0's composed feedback rows, next step
                        sl.each_slab(0, [&](const float* s, int res) { tos.push_back({s, sl.kx[0], res, 1, fbh}); });
                    cand_tiles(pb, metas, in, Wt, l, parts, tos, l == 0 ? pp : nullptr);
                } else if (g.kind == 3) {  // x_pre = ro_const + the shares of every operand but the last layer's state
                    linear_tiles(pb, metas, in, Wt, 64, parts, nullptr, d.ro_const, pm_rm(xpre_rm, (long long)B * 64, 64),
                                 pm_acc(RES_XPRE, 0, 0, 1), sl.frame_tos());
                } else if (fbc) {          // x[t+1] = x_pre + the last layer's share; feeds nothing inside the loop
                    parts.push_back({xpre_rm, RES_XPRE});
                    linear_tiles(pb, metas, in, Wt, 64, parts, nullptr, nullptr, x_next(), pm_acc(RES_X, 1, 0, 1), {});
                } else {
                    linear_tiles(pb, metas, in, Wt, 64, parts, nullptr, d.ro_const, x_next(), pm_acc(RES_X, 1, 0, 1), sl.frame_tos());
                }
            }
        }
        att_rows(pb, metas, 2, 1, attfold);
        std::vector<PmAccess> init = tail(pb);
        pm_prog.att.pp = pp;
        pm_prog.att.pp_st = (long long)hc * B * 32;
        pm_prog.w16 = d.bf16 ? 1 : 0;  // (every piece of a layer product is a PM_GEMM16 unit; the output tiles stay f32)
        if (fbc)  // step 0: zero rows where the last layer's state would go
            sl.each_slab(0, [&](const float* s, int res) {
                pb.add_init(zero_rows, H, H, s, sl.kx[0], fbh);
                init.push_back(pm_acc(res, 0, fbh, hc));
            });
        if (sw_pm_dump_plan())
            for (const PmGroup& g : gs)
                for (const PmPiece& p : g.pc)
                    fprintf(stderr, "[pieces] %s%d phase %d: chunks %d..%d (K %d) %s phase %d lag %d\n",
                            g.kind == 0 ? "G" : (g.kind == 1 ? "C" : (g.kind == 2 ? "OUT" : "XPRE")), g.l, g.slot, p.c0, p.c0 + p.nch, p.nch * 16,
                            p.crit ? "CRITICAL" : "piece", p.slot, p.lag);
        const int n_extra = fbc ? 2 : 1;  // ticks beyond S: main units lag one tick, the output unit of the fbc plan two
        // no grid barriers by default: with the step cut into pieces a phase is ~3 us of fixed latency + a short K
        // walk, and the barrier was a quarter of it (43.0 -> 36.1 us per step at configs[2]); the whole-K plan above
        // measured no gain (57.6 either way).  Bit-identical to the barrier mode (tests/test_gpu_persist.py)
        pm_prog.dataflow = sw_pm_dataflow(1);
        pb.add_fill(part_base, (long long)(part_end - part_base));
        if (fbc) pb.add_fill(xpre_rm, (long long)(S + 1) * B * 64);
        if (attfold) pb.add_fill(pp, (long long)S * hc * B * 32);
        memset(pieces_info, 0, sizeof(pieces_info));
        pieces_info[1] = npart; pieces_info[15] = (fbc ? 1 : 0) + (attfold ? 2 : 0);
        finish(pb, fbc ? PIECES_FBC : PIECES, S + n_extra, check_pieces(metas, init, n_slots, 4, 4 + n_extra));
    }


    void layer_segs(SkJob& j, int l, int t, const float* first, const float* W, int ldw, const float* Wf) const {
        const size_t BH = (size_t)d.B * d.H, BE = (size_t)d.B * d.E;
        const int nxt = (t + 1) & 1;
        int n = 0;
        j.seg[n++] = sk_seg(first, d.H, W, ldw, d.H, 0);
        const float* wsrc = d.w + (size_t)(l == 0 ? t : t + 1) * BE;
        j.seg[n++] = sk_seg(wsrc, d.E, W + (size_t)d.H * ldw, ldw, d.E, 0);
        if (!d.layer_norm) {  // with layer_norm these arrive normalised through the additive input instead
            for (int q = 0; q < l; ++q)
                j.seg[n++] = sk_seg(d.h[q] + nxt * BH, d.H, W + (size_t)(d.H + d.E + q * d.H) * ldw, ldw, d.H, 0);
            if (Wf) j.seg[n++] = sk_seg(d.x + (size_t)t * d.B * d.ldx, d.ldx, Wf, ldw, d.O, 0);
        }
        j.nseg = n;
    }

    // ---- layer_norm: scratch layout and the per-step normalised sums --------------------------------
    int ngrp() const { return d.cell == 1 ? 1 : 2; }
    int gw(int g) const { return d.cell == 1 ? 4 * d.H : (g == 0 ? 2 * d.H : d.H); }
    float* tmp(int g, int k) const {  // k = 0..3 projections, k = 4: the summed additive input
        float* p = d.ln_scratch;
        if (g == 1) p += (size_t)5 * d.B * gw(0);
        return p + (size_t)k * d.B * gw(g);
    }
    float* rtmp(int k) const {  // k = 0..L-1 readout projections, k = L: un-normalised base
        size_t off = (size_t)5 * d.B * gw(0) + (ngrp() == 2 ? (size_t)5 * d.B * gw(1) : 0);
        return d.ln_scratch + off + (size_t)k * d.B * d.R;
    }
    long long scratch_need() const {
        return (long long)5 * d.B * gw(0) + (ngrp() == 2 ? (long long)5 * d.B * gw(1) : 0) +
               (long long)(d.L + 1) * d.B * d.R;
    }

    // Additive inputs of layer l at step t = speaker term + norm(feedback Fork) + sum_j norm(h_j Fork).
    int ln_layer_inputs(int l, int t, hipStream_t st, const float*& addg, const float*& addc) const {
        const size_t BH = (size_t)d.B * d.H;
        const int nxt = (t + 1) & 1;
        SkJob jobs[SK_MAXJOB];
        NormSumGroup grp[2];
        int nj = 0;
        for (int g = 0; g < ngrp(); ++g) {
            const int wd = gw(g);
            const float* W = g == 0 ? d.Wg[l] : d.Wc[l];
            const float* Wf = g == 0 ? d.Wfg[l] : d.Wfc[l];
            NormSumGroup& G = grp[g];
            G.nsrc = 0; G.N = wd;
            G.base = g == 0 ? d.seq_g[l] : d.seq_c[l];
            G.dst = tmp(g, 4);
            if (Wf) {
                SkJob& j = jobs[nj++];
                sk_linear_job(j, sk_seg(d.x + (size_t)t * d.B * d.ldx, d.ldx, Wf, wd, d.O, 0), d.B, wd, d.H, tmp(g, G.nsrc), wd);
                j.bias = g == 0 ? d.bfg[l] : d.bfc[l];
                G.src[G.nsrc++] = j.out;
            }
            for (int q = 0; q < l; ++q) {
                SkJob& j = jobs[nj++];
                sk_linear_job(j, sk_seg(d.h[q] + nxt * BH, d.H, W + (size_t)(d.H + d.E + q * d.H) * wd, wd, d.H, 0), d.B, wd, d.H,
                              tmp(g, G.nsrc), wd);
                const int pj = l * PARROT_MAX_LAYERS + q;
                j.bias = g == 0 ? d.ln_bg[pj] : d.ln_bc[pj];
                G.src[G.nsrc++] = j.out;
            }
        }
        if (nj == 0) return 0;
        PL_TRY(launch_jobs(jobs, nj, st));
        PL_TRY(norm_sum_launch(grp, ngrp(), d.B, PARROT_NORM_EPS, st));
        addg = tmp(0, 4);
        if (ngrp() == 2) addc = tmp(1, 4);
        return 0;
    }

    // readout = att_to_readout(w) + speaker term + sum_l norm(h{l}_to_readout(h_l))   (model.py:992-1006)
    int ln_readout(int t, hipStream_t st) const {
        const size_t BH = (size_t)d.B * d.H, BE = (size_t)d.B * d.E;
        const int nxt = (t + 1) & 1;
        SkJob jobs[PARROT_MAX_LAYERS + 1];
        NormSumGroup G;
        G.nsrc = 0; G.N = d.R; G.base = rtmp(d.L); G.dst = d.readout;
        for (int l = 0; l < d.L; ++l) {
            SkJob& j = jobs[l];
            sk_linear_job(j, sk_seg(d.h[l] + nxt * BH, d.H, d.Wr + (size_t)l * d.H * d.R, d.R, d.H, 0), d.B, d.R, d.H, rtmp(l), d.R);
            j.bias = d.br_l[l];
            G.src[G.nsrc++] = j.out;
        }
        SkJob& b = jobs[d.L];
        sk_linear_job(b, sk_seg(d.w + (t + 1) * BE, d.E, d.Wr + (size_t)d.L * d.H * d.R, d.R, d.E, 0), d.B, d.R, d.H, rtmp(d.L), d.R);
        b.bias = d.br; b.add = d.radd; b.ld_add = d.R;
        PL_TRY(launch_jobs(jobs, d.L + 1, st));
        return norm_sum_launch(&G, 1, d.B, PARROT_NORM_EPS, st);
    }

    // forced frames on the launches: the select behind the step's last kernel, in front of everything that reads x[t + 1]
    int force_frame(int t, hipStream_t st) const {
        if (!forced(d)) return 0;
        const size_t o = (size_t)t * d.B * d.ldx;
        return frame_force_launch(d.x + o + (size_t)d.B * d.ldx, d.own_x + o, d.forced + o, d.n_forced, t, d.B, d.O, d.ldx, st);
    }

    int run_all(hipStream_t st) {
        const size_t BH = (size_t)d.B * d.H, BE = (size_t)d.B * d.E, BA = (size_t)d.B * d.A;
        const int H = d.H;
        for (int t = 0; t < d.S; ++t) {
            const int cur = t & 1, nxt = (t + 1) & 1;
            for (int l = 0; l < d.L; ++l) {
                SkJob j;
                const float* addg = d.seq_g[l];
                const float* addc = d.seq_c[l];
                if (d.layer_norm) PL_TRY(ln_layer_inputs(l, t, st, addg, addc));
                if (d.cell == 1) {
                    sk_lstm_job(j, d.B, H, d.cwork[l] + cur * BH, d.cwork[l] + nxt * BH, d.gwork, d.h[l] + nxt * BH);
                    layer_segs(j, l, t, d.h[l] + cur * BH, d.Wg[l], 4 * H, d.Wfg[l]);
                    j.bias = d.bg[l];
                    j.add = addg; j.ld_add = 4 * H;
                    PL_TRY(launch_jobs(&j, 1, st));
                } else {
                    sk_gru_gates_job(j, d.B, H, d.h[l] + cur * BH, d.zwork, d.rwork, d.rhwork);
                    layer_segs(j, l, t, d.h[l] + cur * BH, d.Wg[l], 2 * H, d.Wfg[l]);
                    j.bias = d.bg[l];
                    j.add = addg; j.ld_add = 2 * H;
                    PL_TRY(launch_jobs(&j, 1, st));

                    sk_gru_cand_job(j, d.B, H, d.h[l] + cur * BH, d.zwork, nullptr, d.h[l] + nxt * BH);
                    layer_segs(j, l, t, d.rhwork, d.Wc[l], H, d.Wfc[l]);
                    j.bias = d.bc[l];
                    j.add = addc; j.ld_add = H;
                    PL_TRY(launch_jobs(&j, 1, st));
                }

                if (l == 0) {
                    AttFwdArgs g{};
                    g.h1 = d.h[0] + nxt * BH; g.ldh = H;
                    g.WattT = d.WattT; g.batt = d.batt;
                    g.kappa_prev = d.kappa + t * BA;
                    g.ctx = d.ctx;
                    g.a_out = d.a + t * BA; g.b_out = d.bwork; g.kappa_out = d.kappa + (t + 1) * BA;
                    g.phi_out = d.phi + (size_t)t * d.B * d.U;
                    g.w_out = d.w + (t + 1) * BE; g.ldw = d.E;
                    g.B = d.B; g.H = H; g.A = d.A; g.U = d.U; g.E = d.E; g.esplit = esplit;
                    g.att_type = d.att_type; g.eps = d.eps; g.alignment = d.alignment;
                    g.sharpening = d.sharpening; g.timing = d.timing;
                    if (has_rows) PL_TRY(att_fwd_rows_launch(g, AttRowCtl{rows.sharpening, rows.timing}, st));
                    else PL_TRY(att_fwd_launch(g, st));
                }
            }
            // readouts (model.py:992-1006) and output (model.py:1008-1013)
            SkJob j;
            if (d.layer_norm) {
                PL_TRY(ln_readout(t, st));
            } else {
                sk_linear_job(j, d.B, d.R, H, d.readout, d.R);
                int n = 0;
                for (int l = 0; l < d.L; ++l)
                    j.seg[n++] = sk_seg(d.h[l] + nxt * BH, H, d.Wr + (size_t)l * H * d.R, d.R, H, 0);
                j.seg[n++] = sk_seg(d.w + (t + 1) * BE, d.E, d.Wr + (size_t)d.L * H * d.R, d.R, d.E, 0);
                j.nseg = n;
                j.bias = d.br; j.add = d.radd; j.ld_add = d.R;
                PL_TRY(launch_jobs(&j, 1, st));
            }

            if (d.gmm_K > 0) {
                // GMM head: three projections of the readout in one launch, then the sampling kernel.
                const int OK = d.O * d.gmm_K;
                SkJob g3[3];
                const float* Ws[3] = {d.Wmu, d.Wsig, d.Wco};
                const float* bs[3] = {d.bmu, d.bsig, d.bco};
                const float* as[3] = {d.add_mu, d.add_sig, d.add_co};
                float* os[3] = {d.gmm_mu, d.gmm_sig, d.gmm_co};
                const int ns[3] = {OK, OK, d.gmm_K};
                for (int q = 0; q < 3; ++q) {
                    sk_linear_job(g3[q], sk_seg(d.readout, d.R, Ws[q], ns[q], d.R, 0), d.B, ns[q], H, os[q], ns[q]);
                    g3[q].bias = bs[q]; g3[q].add = as[q]; g3[q].ld_add = ns[q];
                }
                PL_TRY(launch_jobs(g3, 3, st));
                PL_TRY(gmm_sample_launch(d.gmm_mu, d.gmm_sig, d.gmm_co, d.B, d.O, d.gmm_K, d.sampling_bias, d.eps,
                                         d.unif + (size_t)t * d.B, d.noise + (size_t)t * d.B * d.O,
                                         d.x + (size_t)(t + 1) * d.B * d.ldx, d.ldx,
                                         d.pi_out ? d.pi_out + (size_t)t * d.B * d.gmm_K : nullptr, st,
                                         has_rows ? rows.bias : nullptr));
                PL_TRY(force_frame(t, st));
                continue;
            }
            sk_linear_job(j, sk_seg(d.readout, d.R, d.Wo, d.O, d.R, 0), d.B, d.O, H, d.x + (size_t)(t + 1) * d.B * d.ldx, d.ldx);
            j.bias = d.bo; j.add = d.oadd; j.ld_add = d.O;
            PL_TRY(launch_jobs(&j, 1, st));
            PL_TRY(force_frame(t, st));
        }
        return 0;
    }
};

}  // namespace

extern "C" {


long long parrot_sample_persist_floats(const ParrotSampleDesc* desc) { PH_ENTRY();
    if (!desc || !SamplePlan::persist_eligible(*desc)) return 0;
    return SamplePlan::persist_floats(*desc, pm_max_workgroups());
}
long long parrot_sample_persist_floats_forced(const ParrotSampleForcedDesc* desc) { PH_ENTRY();
    if (!desc) return 0;
    const SampleDescX d(*desc);
    return SamplePlan::persist_eligible(d) ? SamplePlan::persist_floats(d, pm_max_workgroups()) : 0;
}
int parrot_sample_is_persistent(void* plan) {
    const SamplePlan* p = static_cast<SamplePlan*>(plan);
    static const int code[] = {0, 1, 2, 3, 1};  // SamplePlan::Program: NONE, WHOLE, PIECES, PIECES_FBC, LSTM
    return p->live ? code[p->program] : 0;
}
int parrot_sample_is_bf16(void* plan) {
    const SamplePlan* p = static_cast<SamplePlan*>(plan);
    return (p && p->live && p->pm_prog.w16) ? 1 : 0;
}
int parrot_sample_status(void* plan) { PH_ENTRY(); return plan ? static_cast<SamplePlan*>(plan)->persist_status() : PARROT_ERR_BADARG; }
int parrot_sample_stops_early(void* plan) {
    const SamplePlan* p = static_cast<SamplePlan*>(plan);
    return (p && p->stops_early()) ? 1 : 0;
}
int parrot_sample_set_row_controls(void* plan, const float* timing, const float* sharpening, const float* sampling_bias) { PH_ENTRY();
    return plan ? static_cast<SamplePlan*>(plan)->set_row_controls(timing, sharpening, sampling_bias) : PARROT_ERR_BADARG;
}
int parrot_sample_steps_run(void* plan, int* steps) { PH_ENTRY();
    return plan ? static_cast<SamplePlan*>(plan)->steps_run(steps) : PARROT_ERR_BADARG;
}
long long parrot_sample_state_floats(const ParrotSampleDesc* desc) { return desc ? SamplePlan::state_floats(*desc) : 0; }
int parrot_sample_save_state(void* plan, float* state, void* stream) { PH_ENTRY();
    return plan ? static_cast<SamplePlan*>(plan)->save_state(state, (hipStream_t)stream) : PARROT_ERR_BADARG;
}
int parrot_sample_load_state(void* plan, const float* state, void* stream) { PH_ENTRY();
    return plan ? static_cast<SamplePlan*>(plan)->load_state(state, (hipStream_t)stream) : PARROT_ERR_BADARG;
}

// (the entries below and their _forced twins: one body each, on the planners' own descriptor)
static int sample_create(const SampleDescX* desc, void** plan) {
    if (!desc || !plan || desc->S < 1 || desc->B < 1 || bad_dims(desc->L) || desc->ldx < desc->O || desc->eou_extra < 0)
        return PARROT_ERR_BADARG;
    if (SamplePlan::forced(*desc) && (!desc->forced || !desc->n_forced || !desc->own_x)) return PARROT_ERR_BADARG;
    if (SamplePlan::forced(*desc) && desc->bf16) return PARROT_ERR_UNSUPPORTED;  // the kernels with forcing have no bf16 K loop
    SamplePlan* p = new (std::nothrow) SamplePlan();
    if (!p) return PARROT_ERR_BADARG;
    p->d = *desc;
    p->use_graph = desc->use_graph;
    p->esplit = att_default_esplit(desc->B, desc->E);
    if (desc->layer_norm) {
        bool ok = desc->ln_scratch && desc->ln_scratch_floats >= p->scratch_need();
        for (int l = 0; l < desc->L; ++l) ok = ok && desc->br_l[l];
        if (!ok) {
            delete p;
            return PARROT_ERR_BADARG;
        }
    }
    p->build_persist();  // decode on the persistent phase machine when the configuration qualifies
    if (SamplePlan::forced(*desc) && p->live && p->own_rows() != 0) {  // (the kernels with forcing read the row controls)
        delete p;
        return PARROT_ERR_BADARG;
    }
    if (desc->bf16 && !parrot_sample_is_bf16(p)) {  // no machine plan with bf16 operands: refused, never a silent f32 decode
        delete p;
        return PARROT_ERR_UNSUPPORTED;
    }
    if (desc->eou_extra > 0 && !p->stops_early()) {  // the stop exists inside the machine only: refused, never all S steps
        delete p;
        return PARROT_ERR_UNSUPPORTED;
    }
    *plan = p;
    return 0;
}
static int sample_plan_pieces_dry(const SampleDescX* desc, int nwg, int* info16) {
    if (!desc || !info16 || nwg < 1 || desc->S < 1 || desc->B < 1 || bad_dims(desc->L)) return PARROT_ERR_BADARG;
    std::unique_ptr<SamplePlan> p(new (std::nothrow) SamplePlan());
    if (!p) return PARROT_ERR_BADARG;
    p->d = *desc;
    p->plan_persist(true, nwg);
    for (int i = 0; i < 16; ++i) info16[i] = p->pieces_info[i];
    return p->program != SamplePlan::NONE ? 0 : PARROT_ERR_UNSUPPORTED;
}
static int sample_plan_digest_dry(const SampleDescX* desc, int nwg, unsigned long long* digest) {
    if (!desc || !digest || nwg < 1 || desc->S < 1 || desc->B < 1 || bad_dims(desc->L)) return PARROT_ERR_BADARG;
    std::unique_ptr<SamplePlan> p(new (std::nothrow) SamplePlan());
    if (!p) return PARROT_ERR_BADARG;
    p->d = *desc;
    p->plan_persist(true, nwg);
    *digest = p->plan_digest;
    return p->program != SamplePlan::NONE ? 0 : PARROT_ERR_UNSUPPORTED;
}
int parrot_sample_create(const ParrotSampleDesc* desc, void** plan) { PH_ENTRY();
    if (!desc) return PARROT_ERR_BADARG;
    const SampleDescX d(*desc);
    return sample_create(&d, plan);
}
int parrot_sample_create_forced(const ParrotSampleForcedDesc* desc, void** plan) { PH_ENTRY();
    if (!desc) return PARROT_ERR_BADARG;
    const SampleDescX d(*desc);
    return sample_create(&d, plan);
}
int parrot_sample_plan_pieces_dry(const ParrotSampleDesc* desc, int nwg, int* info16) { PH_ENTRY();
    if (!desc) return PARROT_ERR_BADARG;
    const SampleDescX d(*desc);
    return sample_plan_pieces_dry(&d, nwg, info16);
}
int parrot_sample_plan_pieces_dry_forced(const ParrotSampleForcedDesc* desc, int nwg, int* info16) { PH_ENTRY();
    if (!desc) return PARROT_ERR_BADARG;
    const SampleDescX d(*desc);
    return sample_plan_pieces_dry(&d, nwg, info16);
}
int parrot_sample_plan_digest_dry(const ParrotSampleDesc* desc, int nwg, unsigned long long* digest) { PH_ENTRY();
    if (!desc) return PARROT_ERR_BADARG;
    const SampleDescX d(*desc);
    return sample_plan_digest_dry(&d, nwg, digest);
}
int parrot_sample_plan_digest_dry_forced(const ParrotSampleForcedDesc* desc, int nwg, unsigned long long* digest) { PH_ENTRY();
    if (!desc) return PARROT_ERR_BADARG;
    const SampleDescX d(*desc);
    return sample_plan_digest_dry(&d, nwg, digest);
}
int parrot_sample_run(void* plan, void* stream) { PH_ENTRY(); return static_cast<PlanBase*>(plan)->run(0, (hipStream_t)stream); }
int parrot_sample_destroy(void* plan) { PH_ENTRY();
    delete static_cast<PlanBase*>(plan);
    return 0;
}

}  // extern "C"

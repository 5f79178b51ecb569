// Host-side program builder of the persistent phase machine (persist.h), shared by its four planners: the training scan
// (plans.hip, DecoderPlan::build_persist) and the decode programs (plans_decode.hip: whole-K phases, the step cut along K,
// LSTM stacks).  It owns what every program has in common -- the workspace carve-up with its bounds, the descriptor
// constructors, the capacity checks of the fixed-size tables, placement and upload -- so that a planner only says which
// slabs exist and which units run with which operands.  Any take() past the workspace and any append past a table's
// capacity marks the build as failed; finish() then refuses the program and the caller falls back.  A program that
// finish() places also gets a digest of its table and records, which the CPU tests hold the decode planners to.  Nothing
// here is device code; everything has internal linkage like the rest of plans_common.h.
#pragma once
#include "plans_common.h"

namespace {

// Batch rows travel in blocks of 16 (one MFMA tile of rows); a program runs with 1, 2 or 4 of them.
int pm_row_blocks(int B) { return B <= 16 ? 1 : (B <= 32 ? 2 : 4); }
long long pm_rows(int B) { return 16ll * pm_row_blocks(B); }

// What the size queries count for the head of the workspace: sync and debug words, the unit table, alignment slack.
long long pm_header_floats(long long n_units) {
    return PM_SYNC_WORDS + PM_DBG_WORDS + (n_units * (long long)sizeof(PmUnit) + 3) / 4 + 64;
}

PmRM pm_rm(const float* p, long long st, int ld) {
    PmRM r;
    r.p = const_cast<float*>(p); r.st = st; r.ld = ld; r.pad = 0;
    return r;
}

struct PmBuilder {
    const bool dry;  // plan and place only: fake addresses, no device memory is touched (the CPU tests)
    const int B, MB, nwg, n_slots, maxu;
    const long long rows;
    PmProgram& P;    // att, init[] and fill[] are filled through the builder, the header by finish()
    std::vector<PmReq> reqs;
    bool failed = false;
    unsigned long long digest = 0;  // of the placed program (finish); 0 while there is none

    // ws / limit_floats: the caller's workspace; dry runs carve a fake one of the size the size query returns
    PmBuilder(PmProgram& prog, bool dry_, float* ws, long long limit_floats, int B_, int nwg_, int n_slots_, int maxu_)
        : dry(dry_), B(B_), MB(pm_row_blocks(B_)), nwg(nwg_), n_slots(n_slots_), maxu(maxu_), rows(pm_rows(B_)), P(prog),
          base(dry_ ? reinterpret_cast<float*>((uintptr_t)0x10000000) : ws), cur(base), limit(limit_floats) {
        memset(&P, 0, sizeof(P));
        if (n_slots > PM_MAXSLOTS || n_slots * maxu > PM_MAXENT) failed = true;
        sync = reinterpret_cast<unsigned*>(take(PM_SYNC_WORDS + PM_DBG_WORDS));
        unit_bytes = (size_t)n_slots * nwg * maxu * sizeof(PmUnit);
        units_dev = reinterpret_cast<PmUnit*>(take((long long)(unit_bytes + 3) / 4 + 16));
        fm_base = cur;
    }

    // ---- arena (16-byte aligned pieces)
    float* take(long long n) {
        float* p = cur;
        cur += (n + 3) / 4 * 4;
        if (n < 0 || cur - base > limit) failed = true;
        return p;
    }
    float* mark() const { return cur; }
    long long used() const { return (long long)(cur - base); }
    // the fragment-major slabs come first, up to fm_end(): one 32-bit buffer resource addresses the region
    void fm_end() {
        fm_floats = (long long)(cur - fm_base);
        if (fm_floats * 4 >= 0xfff00000ll) failed = true;
    }

    // ---- descriptors
    unsigned boff(const float* p) const { return (unsigned)((p - fm_base) * 4); }  // byte offset inside the slab region
    // chunk `chunk` of the slab (K = ks) of step t + step0
    PmDst dst(const float* slab, long long step0, long long ks, int chunk) const {
        PmDst q;
        q.off = boff(slab + step0 * rows * ks); q.st = (unsigned)(rows * ks * 4); q.nch = (int)(ks / 16); q.chunk = chunk;
        return q;
    }
    // A zeroed request for a GEMM unit of phase `slot` that reads K rows from chunk c0 of `slab` (K = ks per step); critical
    // until the caller says otherwise.
    PmReq gemm(int slot, const float* slab, long long ks, int c0, int K, int lag) const {
        PmReq q;
        memset(&q, 0, sizeof(q));
        q.u.kind = PM_GEMM; q.u.M = B; q.u.w_lds = -1; q.u.lag = lag;
        q.u.a_off = boff(slab); q.u.a_st = (unsigned)(rows * ks * 4); q.u.a_nch = (int)(ks / 16); q.u.a_c0 = c0; q.u.K = K;
        q.slot = slot; q.crit = 1; q.krows = K;
        return q;
    }
    PmReq gemm(int slot, const float* slab, long long ks) const { return gemm(slot, slab, ks, 0, (int)ks, 0); }  // whole K
    void push(const PmReq& q) { reqs.push_back(q); }
    void att_rows(int slot, int lag) {  // the attention: one unit per batch row
        for (int b = 0; b < B; ++b) {
            PmReq q;
            memset(&q, 0, sizeof(q));
            q.u.kind = PM_ATT; q.u.lag = lag; q.u.row = b; q.u.w_lds = -1;
            q.slot = slot; q.crit = 1; q.krows = 0;
            reqs.push_back(q);
        }
    }

    void sample_rows(int slot, int lag, const std::vector<PmDst>& fb) {  // GMM sampling: one unit per batch row, placed alike;
        for (int b = 0; b < B; ++b) {                                     // fb: the fed-back-frame chunks x[t + 1] goes to
            PmReq q;
            memset(&q, 0, sizeof(q));
            q.u.kind = PM_SAMPLE; q.u.lag = lag; q.u.row = b; q.u.w_lds = -1;
            for (const PmDst& f : fb) add_dst(q.u, f);
            q.slot = slot; q.crit = 1; q.krows = 0;
            reqs.push_back(q);
        }
    }

    // ---- bounded appends
    void add_dst(PmUnit& u, const PmDst& q) {
        if (u.ndst >= PM_MAXDST) { failed = true; return; }
        u.dst[u.ndst++] = q;
    }
    void add_operand(PmUnit& u, const PmRM& r) {  // the next free additive input of the unit
        for (PmRM& a : u.add)
            if (!a.p) { a = r; return; }
        failed = true;
    }
    void add_wdst(const PmDst& q) {
        if (P.att.nwdst >= PM_MAXWDST) { failed = true; return; }
        P.att.wdst[P.att.nwdst++] = q;
    }
    void add_init(const float* src, int ld, int K, const float* slab, long long ks, int chunk) {
        if (P.ninit >= PM_MAXINIT) { failed = true; return; }
        PmInit& in = P.init[P.ninit++];
        in.src = src; in.ld = ld; in.K = K; in.dst_off = boff(slab); in.nch = (int)(ks / 16); in.chunk = chunk; in.pad = 0;
    }
    void add_fill(void* p, long long nfloats) {  // dataflow mode: a buffer that starts EMPTY
        if (nfloats <= 0) return;
        if (P.nfill >= PM_MAXFILL) { failed = true; return; }
        P.fill[P.nfill].p = p; P.fill[P.nfill].bytes = nfloats * 4; ++P.nfill;
    }
    void fill_fm() { add_fill(fm_base, fm_floats); }

    // What the attention reads from the plan's descriptor, training or decode (same field names); b, sup, dense and pp are
    // the caller's.
    template <class Desc>
    void att_common(const Desc& d, const float* h1) {
        PmAtt& a = P.att;
        a.h1 = pm_rm(h1, (long long)d.B * d.H, d.H);
        a.WattT = d.WattT; a.batt = d.batt; a.ctx = d.ctx;
        a.kappa = d.kappa; a.a = d.a; a.phi = d.phi; a.w = d.w;
        a.B = d.B; a.H = d.H; a.A = d.A; a.U = d.U; a.E = d.E; a.att_type = d.att_type;
        a.eps = d.eps; a.alignment = d.alignment; a.sharpening = d.sharpening; a.timing = d.timing;
    }

    // Places the requests and, unless dry, uploads the unit table and completes the program header.  True: the program may
    // run (dry: would).  chk: the verdict of the planner's symbolic replay (0 = legal).  info16 (or null) receives what
    // parrot_sample_plan_pieces_dry reports of every plan: [0] phases, [2] chk, [3] units, [4 + phase] units of the phase,
    // [14] units that stream their weights.  `digest` then covers the bytes of the placed table and of P as the planner
    // left it (both zero-filled before they were written; the header is not yet set), and T, n_ticks, n_slots, maxu, nwg:
    // with the dry run's fixed workspace address it names the program a descriptor gets (parrot_sample_plan_digest_dry).
    bool finish(int T, int n_ticks, int chk = 0, int* info16 = nullptr) {
        if (info16 && !failed) {
            info16[0] = n_slots; info16[2] = chk; info16[3] = (int)reqs.size();
            for (const PmReq& q : reqs) info16[4 + q.slot] += 1;
        }
        if (failed || chk != 0) return false;
        std::vector<PmUnit> table;
        if (!pm_place(reqs, n_slots, maxu, nwg, table)) return false;
        if (info16)
            for (const PmUnit& u : table)
                if ((u.kind == PM_GEMM || u.kind == PM_GEMM16) && u.w_lds < 0) info16[14] += 1;
        digest = 14695981039346656037ull;  // FNV-1a, 64 bit
        auto eat = [&](const void* p, size_t n) {
            for (size_t i = 0; i < n; ++i) digest = (digest ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
        };
        eat(table.data(), table.size() * sizeof(PmUnit));
        eat(&P, sizeof(P));
        for (int v : {T, n_ticks, n_slots, maxu, nwg}) eat(&v, sizeof(v));
        if (dry) return true;
        if (hipMemcpy(units_dev, table.data(), unit_bytes, hipMemcpyHostToDevice) != hipSuccess) return false;
        P.T = T; P.n_ticks = n_ticks; P.nwg = nwg; P.MB = MB; P.M = B; P.n_slots = n_slots; P.maxu = maxu;
        P.units = units_dev; P.sync = sync; P.fm_base = fm_base;
        return true;
    }

private:
    float* const base;
    float* cur;
    const long long limit;
    unsigned* sync = nullptr;
    PmUnit* units_dev = nullptr;
    size_t unit_bytes = 0;
    float* fm_base = nullptr;
    long long fm_floats = 0;
};

}  // namespace

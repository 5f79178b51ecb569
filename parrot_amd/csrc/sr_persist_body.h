// The body of the SampleRNN persistent sample kernel, included twice by sr_persist.hip (which describes it): once as
// srp_kernel<D, MG> (SRP_FX false: the kernel as it always was, under the name it always had) and once as
// srp_fx_kernel<D, MG> (SRP_FX true: forced samples, per-sample log-probabilities and the draw statistics compiled in).  Two texts for the
// compiler, not one function called from two kernels: a shared __device__ body changed the register allocation of the
// kernels that use neither facility (srp_kernel<1024, true> went from 16 to 36 bytes of scratch).
template <int D, bool MG>
__global__ __launch_bounds__(SRP_THREADS) void SRP_KERNEL(const SrpArgs a) {
    constexpr bool FX = SRP_FX;
    constexpr int Q = SRP_Q;
    constexpr int DC = D / 32, G = DC / 4, S = SRP_THREADS / G, KP = D / S;
    constexpr int QC = Q / 32, GQ = QC / 4, SQ = SRP_THREADS / GQ, KQ = D / SQ;
    static_assert(KP >= 1 && KQ >= 1 && S * G == SRP_THREADS && S * KP == D, "unsupported width");
    extern __shared__ __attribute__((aligned(16))) char srp_smem[];
    f32x4* act = reinterpret_cast<f32x4*>(srp_smem);       // [D]
    f32x4* red = act + D;                                   // [256]
    f32x4* lg = red + 256;                                  // [Q]   team logits (4 streams per vector)
    float* ev = reinterpret_cast<float*>(lg + Q);           // [4][Q] exp values of the temperature draw
    float* tmp = ev + 4 * Q;                                // [4 * DC] transposition scratch of the gather phase
    float* t2l = tmp + 4 * DC;                              // [Q][DC] this CU's columns of t2tbl[FS-1] (the newest sample's row)
    SrpShared* sh = reinterpret_cast<SrpShared*>(t2l + Q * DC);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* sync = reinterpret_cast<unsigned*>(a.ws);
    unsigned* abort_ = sync + 512;
    unsigned long long* stamps = reinterpret_cast<unsigned long long*>(sync + 600);
    // Team = the XCD this workgroup runs on; rank = its place among the XCD's 32 workgroups.  The dispatcher deals
    // workgroups to the XCDs round-robin -- workgroup i runs on XCD (i + c) % 8 with one c per launch --, so the workgroups
    // with equal blockIdx % 8 share an XCD and blockIdx / 8 numbers them 0 .. 31 without the census atomic of round 5 (a
    // cold L2 round trip in front of every load of the prologue; the census word is still counted, without waiting for
    // it).  c is NOT always 0: tools/xcc_map_probe.hip saw c = 0 in 5200 launches (eager, graphs, odd grids in front), but
    // a check `XCC_ID == blockIdx % 8` placed here aborted 9 of the 28 generation tests that this numbering passes (session
    // r06bv) -- so the team is read from the hardware register, never computed.  A placement that splits a blockIdx % 8
    // class over XCDs leaves a team incomplete: its polls time out and raise abort (the caller falls back to launches).
    const int team = srp_xcc();
    const int cu = (int)(blockIdx.x / SRP_NTEAMS);
    const int ngroups = MG ? a.ngroups : 1;
    bool timing = a.pad && blockIdx.x == 0 && tid == 0;  // (the stamps of a timed launch are group 0's)
    if (timing) stamps[80] = srp_clock();
    if (tid == 0) __hip_atomic_fetch_add(sync + 256 + team * 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);

    // ---- Prologue.  Everything the first step needs is requested before the first wait, in the order of need: the
    // carry of the previous launch (below), the newest sample's table slice (-> LDS), then the weight slices of L3 and
    // Output (-> registers), which the first step's products wait for where they use them.
    //
    // Carry: the sample history of this team and the table part of step 0's gather depend on the samples the PREVIOUS
    // launch produced -- through tbase -> samples -> table rows, three dependent cold round trips.  The previous launch
    // knows all of it when it ends, so its tail leaves both in the workspace (history [4][FS]; per CU the sums
    // [4][DC]) together with the sample index they are for; a launch whose t0 matches takes them from fixed
    // addresses (one round trip beside everything else), any other launch (the first of an utterance) walks the chain.
    // (tbase and the carry's sample index through the scalar cache: not in the queue of the vector loads, whose results
    // return in order -- the weight requests need not wait for them)
    typedef const int __attribute__((address_space(4))) * srp_cint;
    const int t0 = *(srp_cint)(unsigned long long)a.tbase + a.toff;
    // (the draw origin beside it, once per launch: a seeded draw is keyed by the sample's index in the whole run)
    typedef const unsigned long long __attribute__((address_space(4))) * srp_cull;
    const unsigned long long draw0 = *(srp_cull)(unsigned long long)a.origin;
    // Row groups (MG): everything from here to the exchange buffers below that depends on the streams is set for group 0
    // and moved on at the end of the group loop -- srow = the first stream of this team in the current group, its carry
    // block, gb --; the four values requested here (carry_t, hc, cs, f0: what a group starts from) are used up at the top
    // of the loop and asked for again, for the next group, behind the current group's sample steps.
    int* carry = reinterpret_cast<int*>(a.ws + srp_carry_base(D, Q, ngroups)) + (size_t)team * SRP_CARRY_WORDS;
    float* carry_sum = reinterpret_cast<float*>(carry + 16 + SRP_ROWS * SRP_CARRY_HIST) + (size_t)cu * SRP_ROWS * DC;
    int carry_t = *(srp_cint)(unsigned long long)carry;
    // (threads past SRP_ROWS * FS repeat the last slot: same address, same value, same LDS word -- no divergent block the
    // compiler could sink the request into)
    const int hu = min(tid, SRP_ROWS * a.FS - 1), hr = hu / a.FS, hpos = hu % a.FS;
    int hc = carry[16 + hr * SRP_CARRY_HIST + min(hpos, SRP_CARRY_HIST - 1)];
    constexpr int GU = SRP_ROWS * DC, GW0 = (SRP_THREADS - GU) / 64;  // first gathering wave (GU <= 128: waves 6-7 at D = 1024)
    const int gu = min(max(tid - GW0 * 64, 0), GU - 1), gr = gu / DC, gc = gu % DC;
    int srow = team * SRP_ROWS;
    int gb = min(srow + gr, a.B - 1);
    float cs = carry_sum[gu];
    float f0 = a.frame_out[(size_t)gb * a.ldf + cu * DC + gc];
    const int g = (tid >> 3) % G, s = 8 * (tid / (8 * G)) + (tid & 7);
    const int gq = (tid >> 3) % GQ, sq = 8 * (tid / (8 * GQ)) + (tid & 7);
    constexpr int T2V = Q * (DC / 4) / SRP_THREADS;  // f32x4 of the table slice per thread
    static_assert(T2V * SRP_THREADS == Q * (DC / 4), "table slice not a multiple of the workgroup");
    f32x4 tv[T2V];
#pragma unroll
    for (int j = 0; j < T2V; ++j) {
        const int idx = tid + j * SRP_THREADS, q = idx / (DC / 4), c4 = idx % (DC / 4);
        tv[j] = *reinterpret_cast<const f32x4*>(a.t2tbl + ((size_t)(a.FS - 1) * Q + q) * D + cu * DC + 4 * c4);
    }
    // column this thread finishes in the reductions (threads tid < DC / tid < QC)
    const int fin_h = cu * DC + 4 * (tid % G) + tid / G;
    const int fin_q = cu * QC + 4 * (tid % GQ) + tid / GQ;
    const float bias3 = a.b3[min(fin_h, D - 1)];
    const float bias4 = a.b4[min(fin_q, Q - 1)];
    __builtin_amdgcn_sched_barrier(0);
    f32x4 w3[KP], w4[KQ];
#pragma unroll
    for (int kk = 0; kk < KP; ++kk)
        w3[kk] = *reinterpret_cast<const f32x4*>(a.W3 + (size_t)(kk * S + s) * D + cu * DC + 4 * g);
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk)
        w4[kk] = *reinterpret_cast<const f32x4*>(a.W4 + (size_t)(kk * SQ + sq) * Q + cu * QC + 4 * gq);
    __builtin_amdgcn_sched_barrier(0);
    // team exchange buffers ([D] f32x4 each, 4 streams per vector): x1, x2, and the logits ([Q] f32x4); one set per
    // (row group, team), numbered like the carry blocks
    float* xbase = a.ws + SRP_SYNC_WORDS + (size_t)team * srp_team_vecs(D, Q) * 4;
    __amdgpu_buffer_rsrc_t xr = srp_rsrc(xbase);
    f32x4* x1 = reinterpret_cast<f32x4*>(xbase);
    f32x4* x2 = x1 + D;
    f32x4* lb = x2 + D;

    // Slot life cycle.  All slots are EMPTY when a plan is created (srp_init_ws) and every launch leaves them EMPTY again,
    // except the logits of its last step: their owners empty them once they hold the complete x1 of the NEXT launch's
    // first step (every CU that published into it has left the previous launch), like the logits of any other step.
    // (With row groups: per group -- a group's last logits are emptied by the same group of the next launch.)
    // A buffer is emptied by its owner as soon as the owner has taken the NEXT buffer of the chain from all 32 CUs (which
    // proves that all of them are done with this one), always by threads that later publish, behind an
    // s_waitcnt vmcnt(0), something the readers take before they look at the emptied buffer again.  No counted barrier.

    // part_i = frame_out[:, i] + sum_{pos < FS-1} t2tbl[pos][sample[t - FS + pos]] for this CU's DC columns: everything of
    // step i's L2 pre-activation that is known one step early (frame_out carries the composed projection and both
    // biases); threads tid < DC keep it as one f32x4 (4 streams) of column fin_h.
    // The gather: SRP_ROWS * DC sums of FS rows each, by the last waves of the workgroup (the first one publishes and
    // finishes the reductions).  Its rows are REQUESTED right after x1 has been taken and SUMMED behind the L3 product --
    // a memory latency in the product's shadow; requests are unconditional (clamped indices, selected sums): a load
    // inside a divergent block is closed by the compiler with s_waitcnt vmcnt(0).  The sum keeps the order of the
    // positions.  Result transposed through tmp; threads tid < DC pick it up behind the next workgroup barrier.
    f32x4 part = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool gwave = __builtin_amdgcn_readfirstlane(wave) >= GW0, gfast = a.FS - 1 <= SRP_GMAX;
    const bool glane = tid - GW0 * 64 >= 0 && tid - GW0 * 64 < GU;
    float gf = 0.f, gv[SRP_GMAX];
    const __amdgpu_buffer_rsrc_t tr = srp_rsrc(a.t2tbl);
    auto gather_rows = [&](int i) {
        int hq[SRP_GMAX];  // the history in one LDS round trip (left to itself the compiler reads, waits, requests: x 12)
#pragma unroll
        for (int pos = 0; pos < SRP_GMAX; ++pos) hq[pos] = sh->hist[gr][i + max(min(pos, a.FS - 2), 0)];
        __builtin_amdgcn_sched_barrier(0);
        // (buffer loads: table base in scalar registers, the position's table as the scalar offset -- no 64-bit address
        // per position kept alive across the sample loop)
#pragma unroll
        for (int pos = 0; pos < SRP_GMAX; ++pos) {
            const int pp = max(min(pos, a.FS - 2), 0);
            gv[pos] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                tr, (unsigned)(hq[pos] * D + cu * DC + gc) * 4u, (unsigned)(pp * Q * D) * 4u, 0));
        }
    };
    auto gather_request = [&](int i) {
        gf = a.frame_out[(size_t)gb * a.ldf + (size_t)i * D + cu * DC + gc];
        gather_rows(i);
    };
    auto rows_sum = [&](int i, float acc) {
        if (gfast) {
#pragma unroll
            for (int pos = 0; pos < SRP_GMAX; ++pos) acc = pos < a.FS - 1 ? acc + gv[pos] : acc;
        } else {
            for (int pos = 0; pos < a.FS - 1; ++pos)
                acc += a.t2tbl[((size_t)pos * Q + sh->hist[gr][i + pos]) * D + cu * DC + gc];
        }
        return acc;
    };
    auto gather_sum = [&](int i) {
        const float acc = rows_sum(i, gf);
        if (glane) tmp[gc * SRP_ROWS + gr] = acc;
    };
    auto take_part = [&]() { if (tid < DC) part = reinterpret_cast<const f32x4*>(tmp)[fin_h - cu * DC]; };
    if (tid == 0) sh->ok = 1;
#pragma unroll
    for (int j = 0; j < T2V; ++j) reinterpret_cast<f32x4*>(t2l)[tid + j * SRP_THREADS] = tv[j];
    int grp = 0;
    do {
        // ---- one row group: streams srow .. srow + 3 of this team (the last group is usually partial: a stream b >= a.B loads
        // stream a.B - 1's operands and stores nothing; a team without a live stream still runs every hand-off)
        if (carry_t == t0) {
            sh->hist[hr][hpos] = hc;
            if (glane) tmp[gc * SRP_ROWS + gr] = f0 + cs;
        } else {
            const int hv = a.samples[(size_t)min(srow + hr, a.B - 1) * a.len + t0 - a.FS + hpos];
            sh->hist[hr][hpos] = hv;
            __syncthreads();
            if (gwave) {
                gather_request(0);
                gather_sum(0);
            }
        }
        // Per-utterance draws: wave r picks for row srow + r, so it parks that row's entry in the shared block (rows past B:
        // the entry of row B - 1, like every other per-row load here), once per launch and row group -- through the scalar
        // cache like tbase and the draw origin, beside the vector queue.  The branch is uniform; without entries, no code runs.
        if (a.utt && wave < SRP_ROWS) {
            const int rw = __builtin_amdgcn_readfirstlane(wave);
            const unsigned long long ea = (unsigned long long)(a.utt + min(srow + rw, a.B - 1));
            typedef const float __attribute__((address_space(4))) * srp_cfloat;
            const unsigned long long es = *(srp_cull)ea, eo = *(srp_cull)(ea + 8);
            const float et = *(srp_cfloat)(ea + 16);
            const int ek = *(srp_cint)(ea + 20);
            const float ep = *(srp_cfloat)(ea + 24);
            const float em = *(srp_cfloat)(ea + 28);
            // (top_k parked as the pick reads it: 0 = no truncation of any kind, SRP_NUCLEUS set = the row has a nucleus,
            // SRP_MINP set = it has a min_p)
            const int ekn = (ek > 0 && ek < Q ? ek : 0) | (ep > 0.f && ep < 1.f ? SRP_NUCLEUS : 0) |
                            (em > 0.f && em <= 1.f ? SRP_MINP : 0);
            if (lane == 0) {
                sh->useed[rw] = es; sh->uoff[rw] = eo; sh->utemp[rw] = et; sh->utopk[rw] = ekn; sh->utopp[rw] = ep;
                sh->uminp[rw] = em;
            }
        }
        // (no entries: every row draws with the plan's nucleus and the plan's min_p; both stores unconditional)
        if (!a.utt && tid < SRP_ROWS) { sh->utopp[tid] = a.top_p; sh->uminp[tid] = a.min_p; }
        if constexpr (FX) {
            // (the two pointers of the draw statistics, parked like the plan's nucleus: an argument read inside the step
            // loop is scalars carried across it, which srp_fx_kernel<1024, true> pays for in spilled VGPRs)
            if (tid == 0) { sh->dlogp = a.dlogp; sh->kept = a.kept; }
            // the forced codes of this launch's steps, rows past B like every other per-row load here; a value that is no code
            // is parked as -1, so nothing out of range ever reaches the history or a table
            if (a.forced) {
                for (int u = tid; u < SRP_ROWS * a.nsteps; u += SRP_THREADS) {
                    const int fr = u / a.nsteps, fi = u % a.nsteps;
                    const int fv = a.forced[(size_t)min(srow + fr, a.B - 1) * a.len + t0 + fi];
                    sh->forced[fr][fi] = (unsigned)fv < (unsigned)Q ? fv : -1;
                }
            }
        }
        __syncthreads();
        take_part();
        if (timing) stamps[81] = srp_clock();

        auto stamp = [&](int i, int q) { if (timing && i < 10) stamps[i * 8 + q] = srp_clock(); };
        for (int i = 0; i < a.nsteps; ++i) {
            const bool more = i + 1 < a.nsteps;
            stamp(i, 0);
            // ---- x1 = relu(part_i + the newest sample's row): no product, the owner publishes its columns right away
            if (tid < DC) {
                const int c = fin_h - cu * DC;
                f32x4 v = part;
#pragma unroll
                for (int r = 0; r < SRP_ROWS; ++r) v[r] += t2l[sh->hist[r][i + a.FS - 1] * DC + c];
                // (behind the stores that emptied x2: none in front of step 0, whose wait would be for the weight slices)
                if (i > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                x1[fin_h] = (f32x4){fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
            }
            stamp(i, 1);
            {
                for (int k = tid; k < D; k += SRP_THREADS) act[k] = srp_take(xr, (unsigned)(k * 16), abort_, sh);
                __syncthreads();
                if (!sh->ok) return;
                stamp(i, 2);
                // x1(i) complete => every CU is done with the logits of step i-1 (i = 0: of the previous launch's last step)
                if (tid < QC) lb[fin_q] = srp_empty();
                if (more && gwave) gather_request(i + 1);
                f32x4 v;
                srp_layer<KP, G>(act, w3, red, v, tid, SRP_FINE(84));
                if (tid < DC) {
                    v += bias3;
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    x2[fin_h] = (f32x4){fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                }
                stamp(i, 3);
                if (more && gwave) gather_sum(i + 1);
                stamp(i, 4);
            }
            {
                for (int k = tid; k < D; k += SRP_THREADS) act[k] = srp_take(xr, (unsigned)((D + k) * 16), abort_, sh);
                __syncthreads();
                if (!sh->ok) return;
                if (more) take_part();
                stamp(i, 5);
                if (tid < QC) {  // x2(i) complete => every CU is done with x1(i); emptied by the threads that publish lb
#pragma unroll
                    for (int q = 0; q < DC / QC; ++q) x1[cu * DC + tid * (DC / QC) + q] = srp_empty();
                }
                f32x4 v;
                srp_layer<KQ, GQ>(act, w4, red, v, tid, SRP_FINE(88));
                if (tid < QC) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    lb[fin_q] = v + bias4;
                }
#ifdef SRP_FINE_TIMERS
                if (timing && i == 5) stamps[92] = srp_clock();
#endif
            }

            // ---- pick (every CU of the team, identical result): argmax with lowest-index ties, or the seeded draw
            if (tid < Q) lg[tid] = srp_take(xr, (unsigned)((2 * D + tid) * 16), abort_, sh);
            __syncthreads();
            if (!sh->ok) return;
            stamp(i, 6);
            if (tid < DC) x2[fin_h] = srp_empty();  // logits(i) complete => every CU is done with x2(i)
            const int t = t0 + i;
            if (wave < SRP_ROWS) {
                const int r = wave;
                float best;
                const int bi = srp_argmax_row<Q>(lg, r, lane, best);
                int pick = bi;
                // (the row's own temperature with per-utterance entries: rows of one team may mix argmax and draws)
                const float temperature = a.utt ? sh->utemp[r] : a.temperature;
                // (and its own truncation, asked for inside the draws only -- an argmax row runs what it always ran --: a uniform
                // branch of both draws; 0 = off, and the draw runs the instructions it always ran.  One word says all three kinds:
                // the top_k in 1 .. Q-1 or 0, SRP_NUCLEUS where the row has a nucleus, SRP_MINP where it has a min_p --
                // SrpArgs::top_k comes that way from the plan, the entries are parked that way by the prologue -- so a draw
                // without any pays one test for all.  The nucleus and the min_p themselves are always read from the shared
                // block, where the prologue parks the plan's values when there are no entries: an argument of the kernel read
                // inside the step loop is one more scalar carried across it)
                auto row_trunc = [&]() { return __builtin_amdgcn_readfirstlane(a.utt ? sh->utopk[r] : a.top_k); };
                auto row_top_p = [&]() { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sh->utopp[r]))); };
                auto row_min_p = [&]() { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sh->uminp[r]))); };
                unsigned dkeep = 0xfu;  // (FX, the statistics behind the pick: the lane's kept bits of a scan draw)
                if (temperature > 0.f && a.draw_mode == 1) {
                    // wave-parallel draw: lane l owns codes 4 l .. 4 l + 3, terms in registers, no LDS; the key, the counter
                    // and the uniform are the ones of the walk below
                    static_assert(Q == 256, "four codes per lane");
                    const int b = srow + r;
                    const float e0 = expf((lg[4 * lane][r] - best) / temperature), e1 = expf((lg[4 * lane + 1][r] - best) / temperature);
                    const float e2 = expf((lg[4 * lane + 2][r] - best) / temperature), e3 = expf((lg[4 * lane + 3][r] - best) / temperature);
                    unsigned long long key = a.seed ^ (0xBF58476D1CE4E5B9ull * (unsigned long long)(b + 1));
                    unsigned long long ctr = draw0 + (unsigned long long)(t + 1);
                    if (a.utt) { key = sh->useed[r]; ctr -= sh->uoff[r]; }
                    if (const int tr = row_trunc()) {
                        const int tk = tr & (SRP_NUCLEUS - 1);
                        const float tp = tr & SRP_NUCLEUS ? row_top_p() : 0.f;
                        const float tm = tr & SRP_MINP ? row_min_p() : 0.f;
                        // the terms outside the kept set become 0.0f (adding them is exact: the tree and its bounds stand)
                        const unsigned f[4] = {srp_order_image(lg[4 * lane][r]), srp_order_image(lg[4 * lane + 1][r]),
                                               srp_order_image(lg[4 * lane + 2][r]), srp_order_image(lg[4 * lane + 3][r])};
                        // (the lane number is made opaque, as in srp_scan_draw: the code indices and what the selection derives
                        // from them are loop invariants the step loop would otherwise carry in registers)
                        int ln = lane;
                        asm volatile("" : "+v"(ln));
                        const int idx[4] = {4 * ln, 4 * ln + 1, 4 * ln + 2, 4 * ln + 3};
                        unsigned keep = tk ? srp_topk_keep<4>(f, idx, tk) : 0xfu;
                        float mk[4] = {keep & 1u ? e0 : 0.f, keep & 2u ? e1 : 0.f, keep & 4u ? e2 : 0.f, keep & 8u ? e3 : 0.f};
                        if (tp != 0.f) {  // the nucleus of what top-k left: the shortest prefix with p of ITS mass
                            keep &= srp_topp_keep<4>(f, idx, mk, tp);
#pragma unroll
                            for (int j = 0; j < 4; ++j) mk[j] = (keep >> j) & 1u ? mk[j] : 0.f;
                        }
                        if (tm != 0.f) {  // min-p last: of what is left, the codes whose term reaches the bar (one compare each)
                            keep &= srp_minp_keep<4>(mk, tm);
#pragma unroll
                            for (int j = 0; j < 4; ++j) mk[j] = (keep >> j) & 1u ? mk[j] : 0.f;
                        }
                        const float m0 = mk[0], m1 = mk[1], m2 = mk[2], m3 = mk[3];
                        const int lk = keep ? 4 * lane + 31 - __clz((int)keep) : -1;
                        if constexpr (FX) dkeep = keep;
                        pick = srp_scan_draw<true>([&](int j) { return j == 0 ? m0 : j == 1 ? m1 : j == 2 ? m2 : m3; }, 4, lane,
                                                   srp_u01(key, ctr), lk);
                    } else {
                        pick = srp_scan_draw([&](int j) { return j == 0 ? e0 : j == 1 ? e1 : j == 2 ? e2 : e3; }, 4, lane, srp_u01(key, ctr));
                    }
                } else if (temperature > 0.f) {
#pragma unroll
                    for (int m = 0; m < Q / 64; ++m) ev[r * Q + lane + 64 * m] = expf((lg[lane + 64 * m][r] - best) / temperature);
                    if (const int tr = row_trunc()) {
                        const int tk = tr & (SRP_NUCLEUS - 1);
                        const float tp = tr & SRP_NUCLEUS ? row_top_p() : 0.f;
                        const float tm = tr & SRP_MINP ? row_min_p() : 0.f;
                        // the terms outside the kept set are overwritten with 0.0f: the walk adds them, exactly
                        unsigned f[Q / 64];
                        int idx[Q / 64], ln = lane;
                        asm volatile("" : "+v"(ln));  // (opaque: see the scan branch)
#pragma unroll
                        for (int m = 0; m < Q / 64; ++m) { f[m] = srp_order_image(lg[lane + 64 * m][r]); idx[m] = ln + 64 * m; }
                        unsigned keep = tk ? srp_topk_keep<Q / 64>(f, idx, tk) : (1u << (Q / 64)) - 1u;
                        if (tp != 0.f) {  // the nucleus of what top-k left; the lane's terms are read back from where it put them
                            float ek[Q / 64];
#pragma unroll
                            for (int m = 0; m < Q / 64; ++m) ek[m] = (keep >> m) & 1u ? ev[r * Q + lane + 64 * m] : 0.f;
                            keep &= srp_topp_keep<Q / 64>(f, idx, ek, tp);
                        }
                        if (tm != 0.f) {  // min-p last: of what is left, the codes whose term reaches the bar (one compare each)
                            float ek[Q / 64];
#pragma unroll
                            for (int m = 0; m < Q / 64; ++m) ek[m] = (keep >> m) & 1u ? ev[r * Q + lane + 64 * m] : 0.f;
                            keep &= srp_minp_keep<Q / 64>(ek, tm);
                        }
#pragma unroll
                        for (int m = 0; m < Q / 64; ++m)
                            if (!((keep >> m) & 1u)) ev[r * Q + lane + 64 * m] = 0.f;
                        // (the highest kept code, parked in the shared block for the fix-up behind the walk: a value carried
                        // across the walk in a register costs some 45 more parked scalars -- in srp_kernel<1024, true> a fourth
                        // spilled VGPR)
                        const int last = srp_topk_last<Q / 64>(keep, idx);
                        if (lane == 0) sh->ulast[r] = last;
                        if constexpr (FX) {
                            // (the set itself, for the statistics behind the pick: a kept code's term may underflow to 0, so
                            // neither the count nor membership can be read back from the terms)
                            if (sh->dlogp) {
#pragma unroll
                                for (int m = 0; m < Q / 64; ++m) {
                                    const unsigned long long bm = __ballot((keep >> m) & 1u);
                                    if (lane == 0) sh->ukeepm[r][m] = bm;
                                }
                            }
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (lane == 0) {
                        const int b = srow + r;
                        float tot = 0.f;
                        for (int q = 0; q < Q; ++q) tot += ev[r * Q + q];
                        // key = what the counter is hashed with: the plan's seed and the stream, or the utterance's seed alone,
                        // its counter taken back by the run index of the utterance's prefix slot
                        unsigned long long key = a.seed ^ (0xBF58476D1CE4E5B9ull * (unsigned long long)(b + 1));
                        unsigned long long ctr = draw0 + (unsigned long long)(t + 1);
                        if (a.utt) { key = sh->useed[r]; ctr -= sh->uoff[r]; }
                        unsigned long long x = key ^ (0x9E3779B97F4A7C15ull * ctr);
                        x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
                        const float u = (float)((x >> 40) + 0.5) * (1.0f / 16777216.0f) * tot;
                        float c = 0.f;
                        pick = Q - 1;
                        for (int q = 0; q < Q; ++q) {
                            c += ev[r * Q + q];
                            if (u < c) { pick = q; break; }
                        }
                    }
                    // A truncated walk never stops at a code outside the kept set (its term 0.0f does not move c), so Q - 1 from
                    // a kept set without it means that no code satisfied u < c (u01 can be exactly 1.0): the pick is the highest
                    // kept code.  (With Q - 1 kept that is Q - 1 itself.)  Behind the walk, whose text stays as it was.
                    if (row_trunc() && lane == 0 && pick == Q - 1) pick = sh->ulast[r];
                }
                if constexpr (FX) {
                    // a forced step has computed its logits and its pick like any other (a seeded draw is keyed by the
                    // sample's index, so it consumed nothing); the caller's code takes the pick's place from here on
                    if (a.forced) {
                        const int fv = sh->forced[r][i];
                        pick = fv >= 0 ? fv : pick;
                    }
                }
                if (lane == 0) {
                    sh->hist[r][a.FS + i] = pick;
                    const int b = srow + r;
                    if (cu == 0 && b < a.B) a.samples[(size_t)b * a.len + t] = pick;
                }
                if constexpr (FX) {
                    // log softmax(logits)[sample] at temperature 1, whatever the step drew with: the wave holds the row's
                    // logits (four codes per lane), the sum is srp_wave_sum's fixed tree -- the same bits whenever the
                    // logits are the same.  One CU writes.
                    if (a.logp && cu == 0) {
                        static_assert(Q == 256, "four codes per lane");
                        const int sc = __builtin_amdgcn_readfirstlane(pick);  // (lane 0 holds the sample in every mode)
                        const float e01 = __fadd_rn(expf(lg[4 * lane][r] - best), expf(lg[4 * lane + 1][r] - best));
                        const float e23 = __fadd_rn(expf(lg[4 * lane + 2][r] - best), expf(lg[4 * lane + 3][r] - best));
                        const float tot = srp_wave_sum(__fadd_rn(e01, e23));
                        const int b = srow + r;
                        if (lane == 0 && b < a.B) a.logp[(size_t)b * a.len + t] = lg[sc][r] - best - logf(tot);
                    }
                }
                if constexpr (FX) {
                    // what the step drew from (samplernn_generate_set_draw_stats): the size of the kept set and the log of the
                    // written sample's probability under it.  Behind the pick, whose instructions stay as they are: the lane
                    // takes four codes in the draw's own layout (4 l + j in the scan, l + 64 j in the walk), their kept bits
                    // from the register the scan left or from the ballots the walk's selection parked, recomputes the terms
                    // (the same expf of the same argument) and the mass is srp_wave_sum's fixed tree.  One CU writes.
                    if (sh->dlogp && cu == 0) {
                        static_assert(Q == 256, "four codes per lane");
                        const int sc = __builtin_amdgcn_readfirstlane(pick);  // (lane 0 holds the sample in every mode)
                        float dl;
                        int cnt;
                        if (temperature > 0.f) {
                            // (a rolled loop, one code at a time: the weights of both layers are live here, and four
                            // expf side by side spilled 18 more VGPRs in srp_fx_kernel<1024, true>)
                            const bool scan = a.draw_mode == 1;
                            const int tr = row_trunc();
                            const unsigned* km = reinterpret_cast<const unsigned*>(sh->ukeepm[r]);
                            float s = 0.f;  // (0 + e is exact: the lane's terms left to right)
                            bool in = false;
                            cnt = 0;
#pragma unroll 1
                            for (int j = 0; j < 4; ++j) {
                                const int code = scan ? 4 * lane + j : lane + 64 * j;
                                bool k = true;
                                if (tr) k = scan ? (dkeep >> j) & 1u : (km[2 * j + (lane >> 5)] >> (lane & 31)) & 1u;
                                s = __fadd_rn(s, k ? expf((lg[code][r] - best) / temperature) : 0.f);
                                cnt += (int)__popcll(__ballot(k));
                                in = in || (k && code == sc);
                            }
                            const float tot = srp_wave_sum(s);
                            dl = __ballot(in) != 0ull ? (lg[sc][r] - best) / temperature - logf(tot) : -INFINITY;
                        } else {
                            cnt = 1;
                            dl = sc == bi ? 0.f : -INFINITY;
                        }
                        const int b = srow + r;
                        if (lane == 0 && b < a.B) {
                            sh->dlogp[(size_t)b * a.len + t] = dl;
                            sh->kept[(size_t)b * a.len + t] = cnt;
                        }
                    }
                }
            }
            if (a.logits && i == a.nsteps - 1 && cu == 0 && tid < Q) {
#pragma unroll
                for (int r = 0; r < SRP_ROWS; ++r) {
                    const int b = srow + r;
                    if (b < a.B) a.logits[(size_t)b * Q + tid] = lg[tid][r];
                }
            }
            __syncthreads();
            stamp(i, 7);
        }
        // ---- the carry for the next launch (see the prologue): this team's last FS samples and, per CU, the table part of
        // the next launch's first gather -- requested here, stored at the very end
        const bool leave = gfast && a.FS <= SRP_CARRY_HIST;
        // (row groups: what the NEXT group starts from, requested here -- one round trip in the shadow of this group's tail;
        // unconditional: the last group asks for its own values again and nobody uses them)
        const int ngt = MG ? min(grp + 1, ngroups - 1) * SRP_NTEAMS + team : team;
        int* ncarry = reinterpret_cast<int*>(a.ws + srp_carry_base(D, Q, ngroups)) + (size_t)ngt * SRP_CARRY_WORDS;
        float* ncarry_sum = reinterpret_cast<float*>(ncarry + 16 + SRP_ROWS * SRP_CARRY_HIST) + (size_t)cu * SRP_ROWS * DC;
        const int ngb = min(ngt * SRP_ROWS + gr, a.B - 1);
        if (MG) {
            carry_t = *(srp_cint)(unsigned long long)ncarry;
            hc = ncarry[16 + hr * SRP_CARRY_HIST + min(hpos, SRP_CARRY_HIST - 1)];
            cs = ncarry_sum[gu];
            f0 = a.frame_out[(size_t)ngb * a.ldf + cu * DC + gc];
        }
        if (leave && gwave) gather_rows(a.nsteps);
        if (leave && cu == 0) {
            carry[16 + hr * SRP_CARRY_HIST + min(hpos, SRP_CARRY_HIST - 1)] = sh->hist[hr][a.nsteps + hpos];
            if (tid == 0) carry[0] = t0 + a.nsteps;
        }
        if (!leave && cu == 0 && tid == 0) carry[0] = -1;
        // ---- the next frame's frame-tier input for this team's streams (saves the launch that would compute it).  All
        // operands of an item are requested in one batch (unconditional loads, dummy addresses where an operand is absent).
        if (timing) stamps[82] = srp_clock();
        if (a.next_in) {
            constexpr int TW = SRP_GMAX + 1;
            const float half_q = (float)(Q / 2);
            const int NN = a.next_n > 0 ? a.next_n : D, NC = NN / 32;  // this CU's share: NC of the NN columns
            const bool gates = a.next_gpre != nullptr, wfast = a.FS <= TW;
            const float* bias_p = a.next_bias ? a.next_bias : a.next_Win;
            const float* gpre_p = gates ? a.next_gpre : a.next_Win;
            const float* h_p = gates ? a.next_h : a.next_Win;
            for (int idx0 = 0; idx0 < SRP_ROWS * NC; idx0 += SRP_THREADS) {
                const int idx = min(idx0 + tid, SRP_ROWS * NC - 1);
                const int r = idx / NC, col = cu * NC + idx % NC;
                const int b = srow + r, bb = min(b, a.B - 1);
                const bool live = idx0 + tid < SRP_ROWS * NC && b < a.B;
                const bool gcol = gates && col < 2 * D;
                const int hc = col < D ? col : min(col - D, D - 1);
                float wv[TW];
#pragma unroll
                for (int p = 0; p < TW; ++p) wv[p] = a.next_Win[(size_t)min(p, a.FS - 1) * NN + col];
                const float bv = bias_p[col];
                const float av = a.next_add[(size_t)bb * a.next_ld_add + col];
                const float gp = gpre_p[gcol ? (size_t)bb * 2 * D + col : 0];
                const float hv2 = h_p[gcol ? (size_t)bb * D + hc : 0];
                float acc = 0.f;
                if (wfast) {
                    int hq[TW];
#pragma unroll
                    for (int p = 0; p < TW; ++p) hq[p] = sh->hist[r][a.nsteps + min(p, a.FS - 1)];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int p = 0; p < TW; ++p) {
                        const float xf = ((float)hq[p] / half_q - 1.0f) * 2.0f;
                        acc = p < a.FS ? fmaf(xf, wv[p], acc) : acc;
                    }
                } else {
                    for (int p = 0; p < a.FS; ++p) {
                        const float xf = ((float)sh->hist[r][a.nsteps + p] / half_q - 1.0f) * 2.0f;
                        acc = fmaf(xf, a.next_Win[(size_t)p * NN + col], acc);
                    }
                }
                acc += (a.next_bias ? bv : 0.f) + av;
                if (!live) continue;
                if (gcol) {
                    // the recurrent product h . Wg of the NEXT frame's gates is already there (it does not depend on the new
                    // samples: the projection launch made it): finish the gates here -- one launch fewer per frame
                    const float gt = ph_sigmoid(gp + acc);
                    if (col < D) a.next_z[(size_t)b * D + col] = gt;          // update gate
                    else a.next_rh[(size_t)b * D + col - D] = gt * hv2;       // reset gate * h
                } else {
                    a.next_in[(size_t)b * NN + col] = acc;
                }
            }
        }
        if (leave && gwave) {
            const float acc = rows_sum(a.nsteps, 0.f);
            if (glane) carry_sum[gu] = acc;
        }
        if (timing) stamps[83] = srp_clock();
        // The LDS arrays are the next group's as well.  The step loop's last barrier lies in front of the tail, so without this
        // one a wave with no share in the tail (or done with it) would run ahead and overwrite sh->hist / tmp under the tail's
        // reads of sh->hist (next_in items, the slow rows_sum) -- the hazard DESIGN 3.6 describes for the decode machine.
        // This barrier closes it: nobody writes the next group's history before every wave is past the tail and the carry sum.
        if (MG) {
            __syncthreads();
            timing = false;
            srow = ngt * SRP_ROWS;
            carry = ncarry;
            carry_sum = ncarry_sum;
            gb = ngb;
            xbase = a.ws + SRP_SYNC_WORDS + (size_t)ngt * srp_team_vecs(D, Q) * 4;
            xr = srp_rsrc(xbase);
            x1 = reinterpret_cast<f32x4*>(xbase);
            x2 = x1 + D;
            lb = x2 + D;
        }
    } while (MG && ++grp < ngroups);  // row groups (MG = false: no loop at all -- the one-group kernel as it was)
}

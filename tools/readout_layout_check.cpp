// Stand-alone host check of the composed readout path's slice arithmetic and workspace layout
// (parrot_amd/csrc/readout.h).  No device code: build with the host compiler, e.g.
//   g++ -std=c++17 -fsanitize=address,undefined tools/readout_layout_check.cpp -o readout_layout_check
// It sweeps shapes, replays every section of the workspace against the size of the query (a section that overlaps
// another, starts unaligned or ends past the query trips an assertion or the sanitizer), and walks the slices of the
// dW' reduction the way the kernels do.
#include "../parrot_amd/csrc/readout.h"

#include <assert.h>
#include <stdio.h>

#include <vector>

// Small workspaces are replayed float by float; large ones (tens of MB) by their bounds: sections in ascending order.
static void claim(std::vector<unsigned char>& map, long long& next, long long total, long long off, long long n) {
    assert(off % 4 == 0 && off >= next && n >= 0 && off + n <= total);
    next = off + n;
    if (map.empty()) return;
    for (long long i = 0; i < n; ++i) {
        assert(map.at((size_t)(off + i)) == 0);
        map[(size_t)(off + i)] = 1;
    }
}

static long long check_one(long long M, const int* K, int nseg, int R, int O, int slice_rows) {
    ParrotReadoutComposedDesc d = {};
    d.M = M; d.nseg = nseg; d.R = R; d.O = O; d.zero_rows = 3; d.slice_rows = slice_rows; d.nbias = nseg;
    int ktot = 0;
    for (int s = 0; s < nseg; ++s) { d.K[s] = K[s]; d.ldx[s] = K[s] + 4; d.lddx[s] = K[s]; ktot += K[s]; }
    d.ldwr = R; d.ldwo = O; d.ldp = O; d.lddp = O; d.ldgwr = R; d.ldgwo = O;
    RoLayout L;
    const int rc = ro_layout(&d, &L);
    assert(rc == 0);
    assert(L.Ktot == ktot && L.kgroups * 4 * RO_KSTRIP >= ktot && (L.kgroups - 1) * 4 * RO_KSTRIP < ktot);
    // slices: multiples of the LDS chunk, cover [0, M) exactly once, none empty
    assert(L.slice_rows % RO_MCHUNK == 0 && L.slice_rows >= RO_MCHUNK && L.nslice >= 1);
    long long covered = 0;
    for (int s = 0; s < L.nslice; ++s) {
        const long long beg = (long long)s * L.slice_rows;
        const long long end = beg + L.slice_rows < M ? beg + L.slice_rows : M;
        assert(beg < M && end > beg && beg == covered);
        covered = end;
    }
    assert(covered == M);
    if (slice_rows > 0) assert(L.slice_rows >= slice_rows && L.slice_rows < slice_rows + RO_MCHUNK);
    assert(L.gwo_slices >= 1 && (long long)L.gwo_slices * RO_GWO_KROWS >= ktot && (L.gwo_slices - 1) * RO_GWO_KROWS < ktot);
    std::vector<unsigned char> map(L.total <= (1 << 20) ? (size_t)L.total : 0, 0);
    const long long kw = (long long)ktot * RO_NP;
    long long next = 0;
    claim(map, next, L.total, L.Wf, kw);
    claim(map, next, L.total, L.Wb, kw);
    claim(map, next, L.total, L.bp, RO_NP);
    claim(map, next, L.total, L.rbsum, R);
    claim(map, next, L.total, L.dW, kw + RO_NP);
    for (int s = 0; s < L.nslice; ++s) claim(map, next, L.total, L.part + (long long)s * (kw + RO_NP), kw + RO_NP);
    assert(L.gwo % 2 == 0);  // doubles
    claim(map, next, L.total, L.gwo, 2LL * L.gwo_slices * R * RO_NP);
    return L.total;
}

int main() {
    const int segs[][4] = {{16, 0, 0, 0}, {32, 32, 16, 0}, {64, 96, 0, 0}, {256, 256, 128, 0}, {1024, 1024, 256, 0}, {48, 16, 16, 16}};
    const int nsegs[] = {1, 3, 2, 3, 3, 4};
    long long checked = 0;
    for (int c = 0; c < 6; ++c)
        for (long long M : {1LL, 15LL, 63LL, 64LL, 65LL, 130LL, 1000LL, 4097LL, 51200LL})
            for (int R : {1, 72, 256})
                for (int O : {1, 63, 64})
                    for (int sr : {0, 1, 64, 100, 4096}) {
                        check_one(M, segs[c], nsegs[c], R, O, sr);
                        ++checked;
                    }
    // refusals
    ParrotReadoutComposedDesc d = {};
    RoLayout L;
    assert(ro_layout(nullptr, &L) == PARROT_ERR_BADARG);
    assert(ro_layout(&d, &L) == PARROT_ERR_BADARG);
    d.M = 10; d.nseg = 1; d.R = 8; d.O = 65; d.K[0] = 16; d.ldx[0] = 16; d.ldwr = 8; d.ldwo = 65;
    assert(ro_layout(&d, &L) == PARROT_ERR_BADARG);
    d.O = 64; d.ldwo = 64; d.K[0] = 24; d.ldx[0] = 24;
    assert(ro_layout(&d, &L) == PARROT_ERR_BADARG);
    d.K[0] = 16; d.ldx[0] = 16;
    assert(ro_layout(&d, &L) == 0);
    printf("ok: %lld shapes\n", checked);
    return 0;
}

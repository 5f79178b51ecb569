// Host-side arithmetic of the composed readout -> output products (readout.hip): argument checks, the split of the
// dW' reduction along M and the workspace layout.  Plain C++ without device code, so it also builds into a stand-alone
// host program (tools/readout_layout_check.cpp) that runs under the host sanitizers.
#pragma once
#include "../../include/parrot_hip.h"

#include <stdint.h>

#define RO_NP 64          // padded output width: columns O .. 63 of W' and of every tile are zero
#define RO_MROWS 128      // rows of M per workgroup of the forward (8 waves x 16 rows) / data-backward (4 x 32) kernels
#define RO_KSTRIP 64      // rows of dW' per wave of the weight-backward kernel; 4 strips per workgroup
#define RO_MCHUNK 64      // rows of dp staged per LDS round of the weight-backward kernel
#define RO_GWO_KROWS 128  // rows of K per partial tile of the gWo product
#define RO_ZERO_BLOCKS 8  // extra workgroups of the data-backward launch that zero-fill the slot-0 rows

struct RoLayout {
    int Ktot;             // sum of the segments' K
    int kgroups;          // workgroups along K of the weight-backward kernel (4 strips of RO_KSTRIP rows each)
    int slice_rows;       // rows of M per slice of the dW' reduction (a multiple of RO_MCHUNK)
    int nslice;           // slices; partial tile s covers rows [s * slice_rows, min(M, (s + 1) * slice_rows))
    int gwo_slices;       // K slices (RO_GWO_KROWS rows each) of the gWo = Wr^T . dW' product
    // offsets in floats, every one a multiple of 4 (16-byte aligned sections)
    long long Wf, Wb;     // fragment-major copies of W' for the forward / the data-backward kernel, Ktot * 64 each
    long long bp;         // b' [64]
    long long rbsum;      // summed readout bias [R], padded to a multiple of 4
    long long dW;         // dW' [Ktot + 1, 64]: row Ktot holds the column sums of dp
    long long part;       // partial tiles of dW' [nslice, Ktot + 1, 64]
    long long gwo;        // partial tiles of the gWo product, DOUBLES [gwo_slices, R, 64] (two floats each)
    long long total;
};

static inline long long ro_up4(long long n) { return (n + 3) / 4 * 4; }

// 0, or PARROT_ERR_BADARG: sizes and leading dimensions (no pointer is read).
static inline int ro_check_sizes(const ParrotReadoutComposedDesc* d) {
    if (!d) return PARROT_ERR_BADARG;
    if (d->M < 1 || d->M > (1LL << 30)) return PARROT_ERR_BADARG;
    if (d->nseg < 1 || d->nseg > PARROT_READOUT_MAX_SEG) return PARROT_ERR_BADARG;
    if (d->O < 1 || d->O > RO_NP || d->R < 1 || d->zero_rows < 0 || d->slice_rows < 0) return PARROT_ERR_BADARG;
    if (d->nbias < 0 || d->nbias > PARROT_READOUT_MAX_SEG) return PARROT_ERR_BADARG;
    long long ktot = 0;
    for (int s = 0; s < d->nseg; ++s) {
        if (d->K[s] < 16 || d->K[s] % 16) return PARROT_ERR_BADARG;
        if (d->ldx[s] < d->K[s] || d->ldx[s] % 4) return PARROT_ERR_BADARG;
        ktot += d->K[s];
    }
    if (ktot > (1 << 20)) return PARROT_ERR_BADARG;
    if (d->ldwr < d->R || d->ldwo < d->O) return PARROT_ERR_BADARG;
    return 0;
}

// The pointers both directions read: operands, weights, biases.
static inline int ro_check_operands(const ParrotReadoutComposedDesc* d) {
    for (int s = 0; s < d->nseg; ++s)
        if (!d->x[s] || ((uintptr_t)d->x[s] & 15)) return PARROT_ERR_BADARG;
    if (!d->Wr || !d->Wo || !d->bo) return PARROT_ERR_BADARG;
    for (int i = 0; i < d->nbias; ++i)
        if (!d->rb[i]) return PARROT_ERR_BADARG;
    return 0;
}

static inline int ro_layout(const ParrotReadoutComposedDesc* d, RoLayout* L) {
    const int rc = ro_check_sizes(d);
    if (rc) return rc;
    int ktot = 0;
    for (int s = 0; s < d->nseg; ++s) ktot += d->K[s];
    L->Ktot = ktot;
    L->kgroups = (ktot + 4 * RO_KSTRIP - 1) / (4 * RO_KSTRIP);
    long long rows;
    if (d->slice_rows > 0) {
        rows = d->slice_rows;
    } else {
        // two workgroups per CU of a 256-CU device: enough slices to fill the chip, few enough to keep the partial
        // tiles (nslice x Ktot x 64 floats) a small fraction of the operand stream
        long long want = 512 / L->kgroups;
        if (want < 1) want = 1;
        rows = (d->M + want - 1) / want;
    }
    rows = (rows + RO_MCHUNK - 1) / RO_MCHUNK * RO_MCHUNK;
    if (rows > (1 << 30)) return PARROT_ERR_BADARG;
    const long long nslice = (d->M + rows - 1) / rows;
    if (nslice > 65535) return PARROT_ERR_BADARG;  // grid.y
    L->slice_rows = (int)rows;
    L->nslice = (int)nslice;
    L->gwo_slices = (ktot + RO_GWO_KROWS - 1) / RO_GWO_KROWS;
    const long long kw = (long long)ktot * RO_NP;
    long long o = 0;
    L->Wf = o; o += kw;
    L->Wb = o; o += kw;
    L->bp = o; o += RO_NP;
    L->rbsum = o; o += ro_up4(d->R);
    L->dW = o; o += kw + RO_NP;
    L->part = o; o += nslice * (kw + RO_NP);
    L->gwo = o; o += 2LL * L->gwo_slices * d->R * RO_NP;
    L->total = o;
    return 0;
}

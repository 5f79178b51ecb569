// Decode state out and in (parrot_sample_save_state / parrot_sample_load_state, plans_decode.hip): one packed [B, W] f32
// buffer, row b = everything utterance b carries from frame t to frame t + 1,
//   [ x (ldx) | kappa (A) | w (E) | h_0 (H) .. h_{L-1} (H) | c_0 .. c_{L-1} (H each, LSTM only) ].
// Gather reads the pieces where the plan's last run left them, scatter writes them where the next run enters.  One block
// per row and 256-column slice; neighbouring threads touch neighbouring floats on both sides.  A few KB per row, twice
// per segment: plain copies.
#include "elementwise.h"

template <bool GATHER>
__global__ __launch_bounds__(256) void decode_state_kernel(DecodeStateSegs s, float* __restrict__ state) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (b >= s.B || j >= s.W) return;
    int k = 0;
    while (k + 1 < s.n && j >= s.off[k + 1]) ++k;
    float* piece = s.p[k] + (size_t)b * s.wd[k] + (j - s.off[k]);
    float* packed = state + (size_t)b * s.W + j;
    if (GATHER) *packed = *piece;
    else *piece = *packed;
}

static int decode_state_launch(const DecodeStateSegs& s, float* state, bool gather, hipStream_t stream) {
    if (!state || s.n < 1 || s.n > DECODE_STATE_MAXSEG || s.B < 1 || s.B > 65535) return PH_ERR_BADARG;
    int W = 0;
    for (int k = 0; k < s.n; ++k) {  // the pieces tile the row: the kernel's search relies on it
        if (!s.p[k] || s.wd[k] < 1 || s.off[k] != W) return PH_ERR_BADARG;
        W += s.wd[k];
    }
    if (W != s.W) return PH_ERR_BADARG;
    const dim3 grid(ceil_div(W, 256), s.B);
    if (gather) hipLaunchKernelGGL(decode_state_kernel<true>, grid, dim3(256), 0, stream, s, state);
    else hipLaunchKernelGGL(decode_state_kernel<false>, grid, dim3(256), 0, stream, s, state);
    return (int)hipGetLastError();
}

int decode_state_gather_launch(const DecodeStateSegs& s, float* state, hipStream_t stream) {
    return decode_state_launch(s, state, true, stream);
}
int decode_state_scatter_launch(const DecodeStateSegs& s, const float* state, hipStream_t stream) {
    return decode_state_launch(s, const_cast<float*>(state), false, stream);
}

// Staging of SampleRNN conditioning frames from device memory (samplernn_generate_stage_features): rows of a frame store
// gathered by an index table into rows first .. first + rows - 1 of a plan's features [T][B][feat_dim], so that frames a
// decoder left on the device enter the vocoder's ring without a visit to the host.
#include "sr_stage.h"

namespace {

// One output float per lane, flat over rows * B * feat_dim: consecutive lanes store consecutive dwords (feature rows lie
// feat_dim = 63 floats apart, so nothing wider than a dword is aligned) and read consecutive dwords of one source row.
// The 63 lanes of a row read the same table entry (one cache line per 16 rows).  An entry outside 0 .. src_rows-1 is an
// idle slot: zeros, and no address is formed from it.
__global__ __launch_bounds__(256) void sr_stage_features_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                                long long src_rows, int src_ld, const int* __restrict__ index,
                                                                int feat_dim, long long total) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long rb = i / feat_dim;
        const int c = (int)(i - rb * feat_dim);
        const long long row = index[rb];
        dst[i] = row >= 0 && row < src_rows ? src[row * (long long)src_ld + c] : 0.f;
    }
}

}  // namespace

int sr_stage_features(float* features, int B, int feat_dim, const float* src, long long src_rows, int src_ld, const int* index,
                      int first, int rows, hipStream_t stream) {
    const long long total = (long long)rows * B * feat_dim;
    const long long blocks = (total + 255) / 256;
    sr_stage_features_kernel<<<dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream>>>(
        features + (size_t)first * B * feat_dim, src, src_rows, src_ld, index, feat_dim, total);
    return (int)hipGetLastError();
}

// Launcher of the feature staging kernel (sr_stage.hip); the arguments are checked by its C entry (samplernn.hip).
#pragma once
#include "common.h"

int sr_stage_features(float* features, int B, int feat_dim, const float* src, long long src_rows, int src_ld, const int* index,
                      int first, int rows, hipStream_t stream);

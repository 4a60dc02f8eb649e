// argmax.h - the predicted class of a row of logits, shared by the score statistic (score_cifar.hip) and the confusion matrix
// (class_moments.hip) so that both count the same class for the same row.
#pragma once
#include <hip/hip_runtime.h>

// numpy.argmax over z[0..K): the first maximum, a NaN counting as one.  best = z[arg].
__device__ __forceinline__ int ctgan_argmax_first(const float* __restrict__ z, int K, float& best) {
    best = z[0];
    int arg = 0;
    for (int j = 1; j < K; ++j) {
        const float v = z[j];
        if (!(best != best) && (v > best || v != v)) { best = v; arg = j; }
    }
    return arg;
}

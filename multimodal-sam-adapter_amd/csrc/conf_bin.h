// The confidence side of a pixel, shared by csrc/calibrate.hip (reliability bins) and csrc/selective.hip (confusion counts per confidence bin, and the
// thresholded map): ONE definition of the clamp and of the bin, so that the bins, the counts and the map can never disagree at a bin edge.
#pragma once

// NaN, negatives and -0.0 -> 0; above 1 (and +inf) -> 1
__device__ __forceinline__ float conf_clamp(float c) { return c > 0.0f ? (c > 1.0f ? 1.0f : c) : 0.0f; }

// the bin of a CLAMPED confidence: ONE float32 product, truncated, capped at K - 1 (Kf = (float)K)
__device__ __forceinline__ int conf_bin(float c, int K, float Kf) { return min(K - 1, (int)(c * Kf)); }

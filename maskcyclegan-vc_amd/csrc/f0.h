// Pitch tracking (f0_kernels.hip): YIN F0 contours of a bank of utterances on the front-end's frame grid, and F0 statistics along DTW paths.
#pragma once
#include <hip/hip_runtime.h>

#define MCVC_F0_WINDOW 1024                // integration window W
#define MCVC_F0_MAX_LAG 640                // 22050 / 640 = 34.5 Hz
#define MCVC_F0_SUB_FRAMES 8               // frames of one workgroup: a plan tile of 64 is cut into eight of them
#define MCVC_F0_PAIR_COLS 4                // per pair, int64: x frame offset, y frame offset, first path row, path rows

int mcvc_f0_track_launch(const float* wave, long long n_samples, const int* tiles, int n_tiles, int tau_min, int tau_max, float threshold,
                         float* f0, float* aperiodicity, float* cmnd, long long total_frames, hipStream_t s);
int mcvc_f0_stats_launch(const float* fx, long long x_frames, const float* fy, long long y_frames, const int* path, const long long* pairs,
                         int n_pairs, int* counts, float* sums, hipStream_t s);

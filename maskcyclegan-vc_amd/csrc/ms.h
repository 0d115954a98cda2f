// Non-parallel evaluation (ms_kernels.hip): modulation spectra and global variance of a ragged cepstra bank, their mean-log tables over a
// set of utterances and the distance between two sets.  The definitions are in mask_cyclegan_vc/metrics.py and INTEGRATION.md.
#pragma once
#include <hip/hip_runtime.h>

#define MCVC_MS_MAX_FFT 4096               // the longest utterance (= MCVC_DTW_MAX_FRAMES) and the largest zero-padded transform
#define MCVC_MS_MIN_FFT 1024               // n_fft is 1024, 2048 or 4096
#define MCVC_MS_MAX_K 80
#define MCVC_MS_LAUNCHES 8                 // one msd(): 2 x ms_power, 4 x ms_mean_log (P and var of both sets), 2 x ms_distance (MSD, GVD)

int mcvc_ms_table_fill(int n_fft, float* host);            // cos(2 pi j / n_fft), j < n_fft: float64 rounded once
int mcvc_ms_power_launch(const float* cep, long long n_frames, int K, const int* offs_dev, int n_utts, const int* offs_host, int n_fft,
                         const float* table, float* power, float* mean, float* var, hipStream_t s);
int mcvc_ms_mean_log_launch(const float* values, int n, long long R, float floor, float* out, hipStream_t s);
int mcvc_ms_distance_launch(const float* a, const float* b, int K, int n_bins, int n_used, float* per_dim, float* total, hipStream_t s);

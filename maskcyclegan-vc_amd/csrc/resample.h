// Sample-rate conversion (resample_kernels.hip): scipy's polyphase Kaiser filter on a ragged bank of utterances in one launch.
#pragma once
#include <hip/hip_runtime.h>

#define MCVC_RESAMPLE_MAX_FACTOR 640       // largest max(up, down): every pair between 22050 Hz and 8 .. 96 kHz
#define MCVC_RESAMPLE_TILE 1024            // most output samples of one work-list row
#define MCVC_RESAMPLE_TILE_COLS 8          // int32 per row: in_off, n_in, out0, n, q0, r0, 0, 0
#define MCVC_RESAMPLE_SPAN_MAX 16384       // most staged input samples of one row (64 KB of LDS beside a table of at most 55 KB)

long long mcvc_resample_out_samples_of(long long n_in, int up, int down);
long long mcvc_resample_table_floats_of(int up, int down);
int mcvc_resample_pack_host(const float* h, int n_taps, int up, int down, float* table);
int mcvc_resample_plan_host(const int* in_offs, int n_utts, int up, int down, int* out_offs, int* tiles, int max_tiles, int* n_tiles_out);
int mcvc_resample_run_launch(const float* x, long long n_in_total, const int* tiles, int n_tiles, const float* table, int up, int down, float* y,
                             long long n_out_total, hipStream_t s);

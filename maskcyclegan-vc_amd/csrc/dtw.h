// Objective evaluation (dtw_kernels.hip): log-mel -> mel-cepstra projection and batched dynamic time warping, one wavefront per pair.
#pragma once
#include <hip/hip_runtime.h>

// The boundary row a strip hands to the next one (acc fp32 + len int32 per column) lives in static LDS: 8 bytes x 4096 columns = 32 KB
// per wavefront, half of the 64 KB a kernel gets without asking and a fifth of a CU's 160 KB, so several pairs share a CU.
#define MCVC_DTW_MAX_FRAMES 4096
#define MCVC_DTW_MAX_K 80
#define MCVC_DTW_TABLE_COLS 6              // per pair, int64: x offset, Tx, y offset, Ty, direction-byte offset in the workspace (-1: none), path row offset
#define MCVC_CEP_NMEL 80
#define MCVC_CEP_MAX 79                    // c_1 .. c_79 (c_0 is dropped)

int mcvc_cep_basis_fill(int n_cep, float* host);           // [n_cep][80]: rows 1 .. n_cep of the orthonormal DCT-II, float64 rounded once
int mcvc_cep_project_launch(const float* mel, long long n_frames, const float* basis, int n_cep, float* out, hipStream_t s);
// HOST tables in, HOST table out (table may be null: sizes only).  path_rows: sum of Tx + Ty - 1, the capacity the paths are laid out in.
int mcvc_dtw_plan_host(const int* x_offs, const int* y_offs, int n_pairs, int want_path, long long* table, long long* ws_bytes, long long* path_rows);
int mcvc_dtw_run_launch(const float* x, long long x_frames, const float* y, long long y_frames, int K, float scale, const int* x_offs_host,
                        const int* y_offs_host, const long long* table, int n_pairs, float* cost, int* length, int* path, void* ws,
                        long long ws_bytes, hipStream_t s);

// Mel -> linear magnitude by non-negative least squares (melinv_kernels.hip): FISTA from the clamped pseudo-inverse, one launch.
#pragma once
#include <hip/hip_runtime.h>

#define MCVC_MELINV_MAX_ITER 512

long long mcvc_melinv_tables_floats_of();
// pinv [513][80] | step 1 / lambda | beta_k, k < 512 | per bin: first filter, two weights | per filter: first bin, count, offset of its
// weights | the filters' weights, filter after filter in ascending bin order.  MCVC_ERR_INVALID for a basis without that structure.
int mcvc_melinv_tables_fill(const float* host_basis, const float* host_pinv, double lambda, float* host_out);
int mcvc_melinv_solve_launch(const float* logmel, const float* tables, float* mag_out, int B, int T, int n_iter, hipStream_t s);

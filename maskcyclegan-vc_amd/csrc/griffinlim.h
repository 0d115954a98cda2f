// Griffin-Lim log-mel / magnitude -> waveform decoder (griffinlim_kernels.hip): phase reconstruction against the front-end's own STFT.
#pragma once
#include <hip/hip_runtime.h>

#define MCVC_GL_MIN_FRAMES 2               // reflect padding of 384 needs 385 samples: 256 T >= 385
#define MCVC_GL_MAX_FRAMES (1 << 20)
#define MCVC_GL_KIND_LOGMEL 0              // in [B][80][T], log10
#define MCVC_GL_KIND_LINEAR 1              // in [B][513][T], magnitude

int mcvc_gl_out_samples_of(int T);                         // 256 T; 0 when T is refused
int mcvc_gl_launches_of(int n_iter);                       // 2 n_iter + 3; 0 when n_iter < 0
long long mcvc_gl_tables_floats_of();
// inverse basis in lane order | pinv [513][80] | hann^2 [1024] | the front-end's constant operand (audio.h)
void mcvc_gl_tables_fill(const float* host_pinv, float* host_out);
long long mcvc_gl_workspace_floats_of(int B, int T);       // 0 when B or T is refused
int mcvc_gl_decode_launch(const float* in, int in_kind, const float* angles0, const float* tables, float* out, float* ws, long long ws_floats,
                          int B, int T, int n_iter, float momentum, hipStream_t s);

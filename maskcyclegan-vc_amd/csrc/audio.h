// Waveform -> log-mel front-end (audio_kernels.hip): bank of utterances -> [80][total_frames] in one launch.
#pragma once
#include <hip/hip_runtime.h>

#define MCVC_AUDIO_RATE 22050
#define MCVC_AUDIO_NFFT 1024
#define MCVC_AUDIO_HOP 256
#define MCVC_AUDIO_NMEL 80
#define MCVC_AUDIO_TILE_FRAMES 64          // frames of one utterance per workgroup

int mcvc_audio_frames_of(int n_samples);                   // 0: fewer than 385 samples (refused)
long long mcvc_audio_basis_floats_of();
void mcvc_audio_basis_fill(float* host_out);               // DFT basis in lane order | mel table (audio_kernels.hip has the layout)
// host tables: frame_offs [n_utts + 1], tiles [n_tiles][4] (nullable: count only)
int mcvc_audio_plan_host(const int* sample_offs, int n_utts, int* frame_offs, int* tiles, int max_tiles, int* n_tiles_out);
int mcvc_audio_log_mel_launch(const float* wave, long long n_samples, const int* tiles, int n_tiles, const float* basis, float* out,
                              long long total_frames, hipStream_t s);

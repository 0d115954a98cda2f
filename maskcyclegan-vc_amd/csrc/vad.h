// Silence detection (vad_kernels.hip): frame energies and per-utterance maxima of a ragged bank of utterances.
#pragma once
#include <hip/hip_runtime.h>

#define MCVC_VAD_FRAME 2048                // samples of an energy frame (librosa.effects.trim / split default)
#define MCVC_VAD_HOP 512                   // samples between frames: two mel hops
#define MCVC_VAD_TILE_FRAMES 64            // frames of one utterance per workgroup (one work-list row)
#define MCVC_VAD_LAUNCHES 2                // a memset node that zeroes the maxima, then the kernel

long long mcvc_vad_frames_of(long long n_samples);         // 1 + n / 512; 0 for n < 1
// host tables: frame_offs [n_utts + 1], tiles [n_tiles][4] = first sample of the utterance, its length, utterance index, first frame of the
// row in the utterance (nullable: count only)
int mcvc_vad_plan_host(const int* sample_offs, int n_utts, int* frame_offs, int* tiles, int max_tiles, int* n_tiles_out);
int mcvc_vad_energy_launch(const float* wave, long long n_samples, const int* tiles, int n_tiles, const int* frame_offs_dev, int n_utts, float* mse,
                           long long total_frames, float* ref, hipStream_t s);
// the log-mel front-end's work list (audio.h) for segments that lie anywhere in the bank
int mcvc_audio_plan_segments_host(const int* starts, const int* lengths, int n_segs, int* frame_offs, int* tiles, int max_tiles, int* n_tiles_out);

// Waveform -> log-mel front-end (audio_kernels.hip): bank of utterances -> [80][total_frames] in one launch.
#pragma once
#include <hip/hip_runtime.h>

#define MCVC_AUDIO_RATE 22050
#define MCVC_AUDIO_NFFT 1024
#define MCVC_AUDIO_HOP 256
#define MCVC_AUDIO_NMEL 80
#define MCVC_AUDIO_TILE_FRAMES 64          // frames of one utterance per workgroup
#define MCVC_AUDIO_PAD ((MCVC_AUDIO_NFFT - MCVC_AUDIO_HOP) / 2)            // reflect padding each side: an utterance has more than 384 samples

int mcvc_audio_frames_of(int n_samples);                   // 0: fewer than 385 samples (refused)
long long mcvc_audio_basis_floats_of();
void mcvc_audio_basis_fill(float* host_out);               // DFT basis in lane order | mel table (audio_kernels.hip has the layout)
// host tables: frame_offs [n_utts + 1], tiles [n_tiles][4] (nullable: count only)
int mcvc_audio_plan_host(const int* sample_offs, int n_utts, int* frame_offs, int* tiles, int max_tiles, int* n_tiles_out);
int mcvc_audio_log_mel_launch(const float* wave, long long n_samples, const int* tiles, int n_tiles, const float* basis, float* out,
                              long long total_frames, hipStream_t s);

// Entry blockIdx.x of mcvc_audio_plan's work list ([n_tiles][4] = first sample of the utterance in the bank, its length, output column of
// the tile's first frame, first frame in the utterance) as a kernel reads it.  What the plan guarantees is checked again: for a table that
// does not describe this bank nv is 0, and a kernel that leaves on nv < 1 reads and writes nothing.
struct BankTile {
    long long s0, col0;
    int L, t0, T;              // T: frames of the utterance
    int nv;                    // frames of this tile inside the utterance and inside the output, at most MCVC_AUDIO_TILE_FRAMES

    __device__ __forceinline__ BankTile(const int* tiles, long long n_samples, long long total_frames)
    {
        const int4 tile = reinterpret_cast<const int4*>(tiles)[blockIdx.x];
        s0 = tile.x; L = tile.y; col0 = tile.z; t0 = tile.w;
        T = 0; nv = 0;
        if (L < MCVC_AUDIO_PAD + 1 || s0 < 0 || s0 + L > n_samples || t0 < 0 || col0 < 0) return;
        T = (L - MCVC_AUDIO_HOP) / MCVC_AUDIO_HOP + 1;
        long long n = (long long)T - t0;
        if (n > MCVC_AUDIO_TILE_FRAMES) n = MCVC_AUDIO_TILE_FRAMES;
        if (n > total_frames - col0) n = total_frames - col0;
        nv = n < 0 ? 0 : (int)n;
    }
};

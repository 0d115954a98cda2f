// MelGAN decoder, log-mel -> waveform (vocoder_kernels.hip): Generator(input_size 80, ngf 32, n_residual_layers 3) of Kumar et al. 2019
// in fp32, inference only.  42 weight-normed layers run as 30 launches; the layout of the packed weights is in vocoder_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#define MCVC_VOC_NMEL 80
#define MCVC_VOC_HOP 256                   // output samples per mel frame (8 * 8 * 2 * 2)
#define MCVC_VOC_MIN_FRAMES 4              // ReflectionPad1d(3) of the first layer
#define MCVC_VOC_NLAYERS 42                // Conv1d / ConvTranspose1d modules, in state-dict order
#define MCVC_VOC_NLAUNCH 30

// one launch of the decoder
enum VocKind {
    VOC_CONV = 0,      // Conv1d, reflection padding (k - 1) * d / 2, optional LeakyReLU(0.2) on the input
    VOC_CONVT = 1,     // LeakyReLU + ConvTranspose1d(k = 2r, stride r, padding r / 2), r even, as its r output phases
    VOC_STACK = 2,     // W0 @ x0 + W1 @ lrelu(x1) + b0 + b1: the shortcut and the last 1 x 1 of a ResnetBlock as one K = 2 dim product
    VOC_LAST = 3       // LeakyReLU + reflection pad + Conv1d(C, 1, k) + tanh on the vector ALU
};

long long mcvc_voc_layer_packed_floats_of(int kind, int Cin, int Cout, int k, int r);          // 0: not a shape the kernels take
// HOST in, HOST out.  w0 / b0: the layer (VOC_STACK: the shortcut); w1 / b1: VOC_STACK's block.4, else unused
int mcvc_voc_layer_pack_host(int kind, const float* w0, const float* b0, const float* w1, const float* b1, float* packed, int Cin, int Cout, int k, int r);
// x0 [B][Cin][L] (VOC_STACK: x0 and x1 both [B][Cout][L], Cin = Cout); y [B][Cout][r L] (VOC_LAST: [B][L])
int mcvc_voc_layer_launch(int kind, const float* packed, const float* x0, const float* x1, float* y, int B, int Cin, int Cout, int L, int k, int dil, int r,
                          int act_in, hipStream_t s);

long long mcvc_voc_packed_floats_of();
int mcvc_voc_pack_host(const float* const* table, float* packed);                              // table: 42 x (weight, bias), HOST fp32, weight norm folded
long long mcvc_voc_workspace_floats_of(int B, int T);
int mcvc_voc_decode_launch(const float* packed, const float* mel, float* out, float* ws, long long ws_floats, int B, int T, hipStream_t s);

// mcep_host.h -- the mel-cepstrum's host arithmetic (include/world_hip.h: world_hip_sp2mc states the rule; tables.cpp
// implements it).  No GPU, no HIP type, no other header of the library: a plain program can include this, link tables.cpp
// and call these.
#pragma once

namespace world_hip {

constexpr int kMcepMaxOrder = 255;
constexpr double kMcepMaxAlpha = 0.9;
// i / 1000, i the first of 0 .. 999 whose all-pass warp lies closest (RMS over 1000 points) to the mel curve of fs; NaN for fs < 1
double mcep_alpha(int fs);
// nullptr, or why (fft_size, order, alpha) is refused (a static buffer of the calling thread)
const char *mcep_shape(int fft_size, int order, double alpha);
// M [order + 1][fft_size / 2 + 1]: mc = M ln sp.  The rows are cosine transforms of freqt's rows, made by a long-double
// FFT: milliseconds at any shape
void build_mcep_encode(int fft_size, int order, double alpha, double *M);
// D [fft_size / 2 + 1][order + 1]: ln sp = D mc
void build_mcep_decode(int fft_size, int order, double alpha, double *D);

}  // namespace world_hip

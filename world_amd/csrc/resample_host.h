// resample_host.h -- the resampler's host arithmetic (include/world_hip.h: world_hip_resample_batch states the rule;
// tables.cpp implements it).  No GPU, no HIP type, no other header of the library: a plain program can include this, link
// tables.cpp and call these.  (A header of its own and not part of tables.h, which every kernel unit includes.)
#pragma once

namespace world_hip {

struct ResampleDesign { int zeros; double rolloff, beta; };
struct ResampleShape { long long L, M, W; };       // fs_out / g, fs_in / g, taps on each side
constexpr int kResampleMaxTaps = 4096;             // 2 W
constexpr long long kResampleMaxCoefs = 1LL << 21; // L * 2 W
int resample_length(long long n_in, long long fs_in, long long fs_out);               // ceil(n_in L / M), or -1
// nullptr and *shape filled, or why the rates / design are refused (a static buffer of the calling thread)
const char *resample_shape(long long fs_in, long long fs_out, const ResampleDesign &d, ResampleShape *shape);
void build_resample_taps(const ResampleShape &s, const ResampleDesign &d, double *table);   // [L][2 W], row p

}  // namespace world_hip

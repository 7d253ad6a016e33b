// resample.h -- what api.hip and pcm.hip share about the resampler's kernels (world_hip_resample_batch; resample.inc);
// the host arithmetic is resample_host.h.
#pragma once
#include "devrt.h"
#include "resample_host.h"

namespace world_hip {

// Utterance u: x_len[u] samples of x ([n_utt][x_stride]) -> n_out[u] samples of y ([n_utt][y_stride]).  coef is the
// coefficient table as the device reads it, [2 W][L] with column r = m mod L (the host's [p][i] table, transposed and
// with its rows permuted by p = r M mod L); kdiv[r] = (r M) div L.  Both are unused (nullptr) for the copy of equal rates.
struct ResampleParams {
  int L, M, W;
  int tile, span;                   // outputs per workgroup; doubles staged per workgroup (resample_plan)
  int x_stride, y_stride;
  const double *x;
  double *y;
  const int *x_len, *n_out;         // [n_utt] (device)
  const double *coef;
  const int *kdiv;
};
struct ResamplePlan {
  int tile, span, lds_doubles;
  bool decim, pad;                  // L == 1; and its LDS padded against bank conflicts (M a multiple of 4)
};
ResamplePlan resample_plan(long long L, long long M, long long W);
void launch_resample(const ResampleParams &p, const ResamplePlan &pl, int max_out, int n_utt, hipStream_t stream);
void launch_resample_copy(const ResampleParams &p, int max_len, int n_utt, hipStream_t stream);

}  // namespace world_hip

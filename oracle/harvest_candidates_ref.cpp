// harvest_candidates_ref.cpp -- TEST INFRASTRUCTURE ONLY: the reference's own candidate stage behind a C interface.
//
// GetF0CandidateContour, DetectOfficialF0Candidates and ZeroCrossingEngine live in the reference's harvest.cpp as static
// functions.  This unit includes that file WHERE IT LIES (oracle/Makefile names it in WORLD_REF_HARVEST_CPP; nothing of it is
// copied here) and calls them on zero-crossing lists a test made up, so that tests/test_harvest_candidates_cpu.py holds the
// oracle's restatement (world_oracle.c: wo_harvest_candidates) and the kernels to the reference itself rather than to our
// reading of it.
#include WORLD_REF_HARVEST_CPP

namespace {
// One family's intervals from its fine edges: the two expressions ZeroCrossingEngine ends with (harvest.cpp:189-190), restated
// because the function computes the edges from a signal; ref_zero_crossing_engine below ties the restatement to the function.
int fill(const double *fine_edges, int count, double fs, double *interval_locations, double *intervals) {
  if (count < 2) return 0;
  for (int i = 0; i < count - 1; ++i) {
    intervals[i] = fs / (fine_edges[i + 1] - fine_edges[i]);
    interval_locations[i] = (fine_edges[i] + fine_edges[i + 1]) / 2.0 / fs;
  }
  return count - 1;
}
}  // namespace

// edges [nch][4][ev_cap] fine edges per band and family (falling, rising, peaks, dips: GetFourZeroCrossingIntervals' order),
// counts [nch][4] -> raw [nch][nf] by GetF0CandidateContour on temporal positions i * 1.0 / 1000.0, cand [nf][nch] (rows nch
// wide: DetectOfficialF0CandidatesSub2 does not check its cap) by DetectOfficialF0Candidates with max_candidates = maxc;
// returns its result.  edges == 0: raw is given.
extern "C" int ref_harvest_candidates(const double *edges, const int *counts, int ev_cap, double afs, const double *band_f0,
                                      int nch, int nf, double f0_floor, double f0_ceil, int maxc, double *raw, double *cand) {
  double *tpos = new double[nf];
  for (int i = 0; i < nf; ++i) tpos[i] = i * 1.0 / 1000.0;
  double **rows = new double *[nch], **cands = new double *[nf];
  for (int j = 0; j < nch; ++j) rows[j] = raw + static_cast<size_t>(j) * nf;
  for (int i = 0; i < nf; ++i) cands[i] = cand + static_cast<size_t>(i) * nch;
  if (edges)
    for (int j = 0; j < nch; ++j) {
      ZeroCrossings z = {0};
      const int *n = counts + j * 4;
      const double *e = edges + static_cast<size_t>(j) * 4 * ev_cap;
      z.negative_interval_locations = new double[n[0] + 1]; z.negative_intervals = new double[n[0] + 1];
      z.positive_interval_locations = new double[n[1] + 1]; z.positive_intervals = new double[n[1] + 1];
      z.peak_interval_locations = new double[n[2] + 1]; z.peak_intervals = new double[n[2] + 1];
      z.dip_interval_locations = new double[n[3] + 1]; z.dip_intervals = new double[n[3] + 1];
      z.number_of_negatives = fill(e, n[0], afs, z.negative_interval_locations, z.negative_intervals);
      z.number_of_positives = fill(e + ev_cap, n[1], afs, z.positive_interval_locations, z.positive_intervals);
      z.number_of_peaks = fill(e + 2 * static_cast<size_t>(ev_cap), n[2], afs, z.peak_interval_locations, z.peak_intervals);
      z.number_of_dips = fill(e + 3 * static_cast<size_t>(ev_cap), n[3], afs, z.dip_interval_locations, z.dip_intervals);
      GetF0CandidateContour(&z, band_f0[j], f0_floor, f0_ceil, tpos, nf, rows[j]);
      DestroyZeroCrossings(&z);
    }
  const int nc = DetectOfficialF0Candidates(rows, nch, nf, maxc, cands);
  delete[] rows;
  delete[] cands;
  delete[] tpos;
  return nc;
}

// ZeroCrossingEngine itself on a signal -> locations, intervals [y_length]; returns the number of intervals
extern "C" int ref_zero_crossing_engine(const double *signal, int y_length, double fs, double *locations, double *intervals) {
  return ZeroCrossingEngine(signal, y_length, fs, locations, intervals);
}

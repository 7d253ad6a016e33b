// harvest_refine_ref.cpp -- TEST INFRASTRUCTURE ONLY: the reference's own refinement stage behind a C interface.
//
// OverlapF0Candidates, RefineF0Candidates and GetRefinedF0 live in the reference's harvest.cpp as static functions.  This unit
// includes that file WHERE IT LIES (oracle/Makefile names it in WORLD_REF_HARVEST_CPP; nothing of it is copied here) and calls
// them on a signal and a candidate map a test made up, so that tests/test_harvest_refine_cpu.py holds the oracle's statements
// (world_oracle.c: wo_harvest_refine) and the kernels to the reference itself rather than to our reading of it.
#include WORLD_REF_HARVEST_CPP

// cand [nf][nc] candidates per 1 ms frame (0: none) -> refined, score [nf][7 nc]: the rows HarvestGeneralBody hands on, slot
// j + nc m from OverlapF0Candidates, refined in place by RefineF0Candidates on temporal positions i * 1.0 / 1000.0
extern "C" void ref_harvest_refine(const double *y, int y_len, double afs, const double *cand, int nf, int nc, double f0_floor,
                                   double f0_ceil, double *refined, double *score) {
  if (nc == 0) return;
  const int slots = 7 * nc;
  double *tpos = new double[nf];
  double **rows = new double *[nf], **scores = new double *[nf];
  for (int i = 0; i < nf; ++i) {
    tpos[i] = i * 1.0 / 1000.0;
    rows[i] = refined + static_cast<size_t>(i) * slots;
    scores[i] = score + static_cast<size_t>(i) * slots;
    for (int j = 0; j < slots; ++j) rows[i][j] = j < nc ? cand[static_cast<size_t>(i) * nc + j] : 0.0;
    for (int j = 0; j < slots; ++j) scores[i][j] = 0.0;
  }
  OverlapF0Candidates(nf, nc, rows);
  RefineF0Candidates(y, y_len, afs, tpos, nf, slots, f0_floor, f0_ceil, rows, scores);
  delete[] rows;
  delete[] scores;
  delete[] tpos;
}

// GetRefinedF0 itself on one candidate at one position
extern "C" void ref_harvest_refine_one(const double *y, int y_len, double afs, double pos, double f0, double f0_floor, double f0_ceil,
                                       double *refined, double *score) {
  GetRefinedF0(y, y_len, afs, pos, f0, f0_floor, f0_ceil, refined, score);
}

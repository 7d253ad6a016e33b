// harvest_contour_ref.cpp -- TEST INFRASTRUCTURE ONLY: the reference's own contour stage behind a C interface.
//
// The functions of Harvest's back half (RemoveUnreliableCandidates, SearchF0Base, FixStep1 .. 4, FixF0Contour,
// SmoothF0Contour) live in an anonymous namespace of the reference's harvest.cpp.  This unit includes that file WHERE IT
// LIES (oracle/Makefile names it in WORLD_REF_HARVEST_CPP; nothing of it is copied here) and calls them on candidate maps
// a test made up, so that tests/test_harvest_contour_cpu.py holds the oracle's restatement (world_oracle.c:
// wo_harvest_contour) and the kernels to the reference itself rather than to our reading of it.
#include WORLD_REF_HARVEST_CPP

namespace {
struct Rows {                       // [nf][nslot] as the double ** the reference takes
  double **row;
  int nf;
  Rows(const double *flat, int nf_, int nslot) : row(new double *[nf_]), nf(nf_) {
    for (int i = 0; i < nf; ++i) {
      row[i] = new double[nslot > 0 ? nslot : 1]();
      for (int j = 0; j < nslot; ++j) row[i][j] = flat[static_cast<size_t>(i) * nslot + j];
    }
  }
  void store(double *flat, int nslot) const {
    for (int i = 0; i < nf; ++i)
      for (int j = 0; j < nslot; ++j) flat[static_cast<size_t>(i) * nslot + j] = row[i][j];
  }
  ~Rows() {
    for (int i = 0; i < nf; ++i) delete[] row[i];
    delete[] row;
  }
};
}  // namespace

// cand, score [nf][nslot] refined candidates at 1 ms -> pruned_cand, pruned_score [nf][nslot]; step2, step3, step4 [nf]: the
// stages of FixF0Contour called one by one with FixF0Contour's arguments; whole [nf]: FixF0Contour itself (the caller asserts
// whole == step4); smooth [nf]: SmoothF0Contour of `whole` (frames it does not write are 0, as HarvestGeneralBody's are)
extern "C" void ref_harvest_contour(const double *cand, const double *score, int nf, int nslot, double *pruned_cand,
                                    double *pruned_score, double *step2, double *step3, double *step4, double *whole,
                                    double *smooth) {
  Rows c(cand, nf, nslot), s(score, nf, nslot);
  RemoveUnreliableCandidates(nf, nslot, c.row, s.row);
  c.store(pruned_cand, nslot);
  s.store(pruned_score, nslot);
  double *base = new double[nf], *step1 = new double[nf];
  SearchF0Base(c.row, s.row, nf, nslot, base);
  FixStep1(base, nf, 0.008, step1);
  FixStep2(step1, nf, 6, step2);
  FixStep3(step2, nf, nslot, c.row, 0.18, s.row, step3);
  FixStep4(step3, nf, 9, step4);
  FixF0Contour(c.row, s.row, nf, nslot, whole);
  for (int i = 0; i < nf; ++i) smooth[i] = 0.0;
  SmoothF0Contour(whole, nf, smooth);
  delete[] base;
  delete[] step1;
}

// SmoothF0Contour alone: frames outside the voiced sections of f0 are 0
extern "C" void ref_smooth_f0(const double *f0, int nf, double *smooth) {
  for (int i = 0; i < nf; ++i) smooth[i] = 0.0;
  SmoothF0Contour(f0, nf, smooth);
}

// fft_probe.h -- launchers of the stand-alone transform kernels (fft_probe.hip, fft_probe_swz1.hip: fft_probe_routes.inc)
#pragma once
#include "devrt.h"
#include "tables.h"

namespace world_hip {
bool fft_probe_has_static(int lgn, int max_lr);
void launch_fft_probe(bool inverse, int lgn, int max_lr, int threads, bool static_plan, long batch, const void *d_in,
                      void *d_out, const Tables &tab, hipStream_t stream);

// the compositions of fft.h's entry points that world_hip_probe_fft runs (include/world_hip.h documents them)
enum FftProbeMode : int {
  kFpRfft = 1,             // block_rfft<max_lr>, the table of the inner transform
  kFpIrfft = 2,            // block_irfft<max_lr>
  kFpRfftFrom = 3,         // block_rfft_from<3>
  kFpRfftFullTable = 4,    // block_rfft<4>, the table at the transform's own length
  kFpCfft = 5,             // block_cfft_dif<4>, default plan
  kFpCfftFrom = 6,         // block_cfft_dif_from<3>, input zero beyond N/2
  kFpRfftStatic = 7,       // block_rfft<3, LGN>
  kFpIrfftStatic = 8,      // block_irfft<3, LGN>
  kFpRfftFromStatic = 9,   // block_rfft_from<3, LGN>
  kFpRfftItems = 10,       // block_cfft_dif_static<11, 3, 256> + rfft_merge_items<5, 256>
  kFpIrfftItemsRot = 11,   // irfft_pretwiddle_items_w<5, 256> (rotation twiddles) + block_cfft_dit_static<11, 3, 256>
  kFpIrfftItems = 12,      // irfft_pretwiddle_items<5, 256> + block_cfft_dit_static<11, 3, 256>
  kFpRfftRotTwice = 13,    // block_cfft_dif_static<11, 3, 256> + rfft_merge_items_w<5, 256, true> (rotation twiddles): 2 X
  kFpD4cRfft = 14,         // d4c_frame's staging + block_cfft_dif_static<lg-1, 3, N/16> + rfft_merge_items_rot<K, N/16>
  kFpD4cRfftTwice = 15,    // ... rfft_merge_items_rot<K, N/16, true>: 2 X
  kFpD4cRfftRunTime = 16,  // ... with block_cfft_dif<3> (the run-time plan) for the static stages
  kFpD4cTwiddles = 17,     // the twiddles d4c_frame's staging serves
  kFpDft8 = 18,            // dft8<true> on rows of 8
  kFpDft8Head2 = 19,       // dft8_head2<true> on the first two of a row of 8
};
// one per slot swizzle (fft.h: WH_SWZ); false = the unit has no such composition
bool launch_fft_routes_swz0(int mode, int lgn, int max_lr, int threads, long batch, const void *d_in, void *d_out, const Tables &tab,
                            hipStream_t stream);
#ifdef WORLD_EMU
// (the host emulation has this unit only where tests/emu builds it into the lock-step library: absent = unsupported)
__attribute__((weak))
#endif
bool launch_fft_routes_swz1(int mode, int lgn, int max_lr, int threads, long batch, const void *d_in, void *d_out, const Tables &tab,
                            hipStream_t stream);
}

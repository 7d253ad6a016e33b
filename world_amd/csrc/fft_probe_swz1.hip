// fft_probe_swz1.hip -- the probe kernels of fft_probe_routes.inc under the LDS slot swizzle that d4c.hip alone compiles
// (fft.h: WH_SWZ 1): what d4c_lovetrain and d4c_frame run of fft.h, in isolation.  Test and measurement hook like
// fft_probe.hip; replaces nothing in the reference.
#define WH_SWZ 1
#include "fft_probe_routes.inc"

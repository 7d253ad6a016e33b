// d4c_select_probe.h -- launcher of the band selection's stand-alone kernel (d4c.hip: d4c_select_probe; a header of its own so
// that no other unit's object changes with it)
#pragma once
#include "devrt.h"

namespace world_hip {
// rows workgroups of `threads` threads: keys [rows][threads][10] -> out [rows][3] (include/world_hip.h: world_hip_probe_select).
// false: `threads` is not one of d4c_frame's workgroup sizes
bool launch_d4c_select_probe(int mode, int threads, int K, long rows, const double *d_keys, double *d_out, hipStream_t stream);
}

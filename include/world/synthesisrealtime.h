/* world/synthesisrealtime.h -- drop-in for the reference header of the same name: a caller that says
 * #include "world/synthesisrealtime.h" compiles against this repository's include/ directory unchanged.
 * Declares WorldSynthesizer, InitializeSynthesizer, AddParameters, RefreshSynthesizer, DestroySynthesizer, IsLocked
 * and Synthesis2 (reference src/world/synthesisrealtime.h); all declarations live in ../world_hip.h (Part 1), which
 * states where this library's synthesiser differs from the reference's. */
#ifndef WORLD_HIP_FORWARD_SYNTHESISREALTIME_H_
#define WORLD_HIP_FORWARD_SYNTHESISREALTIME_H_
#include "../world_hip.h"
#endif

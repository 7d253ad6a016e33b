// emu_rt.cpp -- runtime half of the host emulation of world_amd/csrc/devrt.h
// (TEST INFRASTRUCTURE: lets `pytest -m "not gpu"` run the kernels' logic on the
// CPU, one thread per block; never part of libworld_hip.so).
#include "devrt.h"

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
thread_local char *emu_lds_base = nullptr;

namespace devrt {
// Poison: kernels must not rely on zero-initialised or left-over workspace.  0xFF bytes, because almost everything here is
// a double: they read as a NaN (as -1 / UINT_MAX where an index or a count is read), where the 0xA5 used before read
// as -2e-127 and vanished in any sum.  devrt::dpoison is the -DWH_HBM_POISON build's primitive, unconditional under WORLD_EMU
// (devrt.h defines it there): the library calls it at every carve, so every emulated stage starts on a freshly poisoned arena.
void *dmalloc(size_t bytes) {
  void *p = malloc(bytes ? bytes : 1);
  dpoison(p, bytes, nullptr);
  return p;
}
void dfree(void *p) { free(p); }
static thread_local char *lds_block = nullptr;
void emu_run_begin(size_t lds_bytes) {
  lds_block = static_cast<char *>(malloc(lds_bytes + 64));
  memset(lds_block, 0xFF, lds_bytes + 64);
  emu_lds_base = lds_block;
}
void emu_run_end() {
  free(lds_block);
  lds_block = nullptr;
  emu_lds_base = nullptr;
}
}  // namespace devrt

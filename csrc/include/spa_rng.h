// Counter-based RNG shared by the kernels that draw uniforms (misc.hip: VAE reparameterisation;
// sample.hip: token sampling). u01(seed, i) is a pure function of its arguments, so a draw is
// reproducible on the host (solvingpapers_amd/ops/sampling.py::u01 is the exact Python twin).
#pragma once

#include <cstdint>

namespace spa {

__device__ __forceinline__ uint32_t mix32(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return (uint32_t)k;
}
__device__ __forceinline__ float u01(uint64_t seed, uint64_t i) {  // (0, 1]
  return ((float)(mix32(seed * 0x9E3779B97F4A7C15ULL + i) >> 8) + 1.f) * (1.f / 16777216.f);
}

}  // namespace spa

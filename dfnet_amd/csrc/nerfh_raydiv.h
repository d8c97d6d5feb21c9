// nerfh_raydiv.h — point index -> ray index without an integer division (kernel variant 12, nerfh_mlp_lean.hip).
// Host and device; free of HIP, so that a plain C++ program can include it (tests/test_ray_div_magic.py).
//
// A launch indexes its points with q < 2^31 (launch_tiles) and divides them by n = samples per ray, which is the same for every lane of
// every wave.  For n >= 2 let s = ceil(log2 n), so 2^(s-1) < n <= 2^s, and m = ceil(2^(31+s) / n).  Then 2^31 <= m < 2^32 (m fits 32
// bits), m n = 2^(31+s) + e with 0 <= e < n <= 2^s, and
//     q m / 2^(31+s) = q / n + q e / (n 2^(31+s)),   where q e / 2^(31+s) < 2^31 2^s / 2^(31+s) = 1,
// so the second term is below 1 / n and cannot carry q / n over the next integer: floor(q m / 2^(31+s)) = floor(q / n).  The left side is
// (the high word of the 32 x 32 -> 64-bit product) >> (s - 1): one v_mul_hi_u32 and one shift.  n = 1 has no such m (it would be 2^32):
// magic 0 marks it and the quotient is q itself.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DFN_RAYDIV_HD __host__ __device__ inline
#else
#define DFN_RAYDIV_HD inline
#endif

namespace dfn {

struct RayDiv {
  uint32_t magic;   // m; 0: n == 1
  uint32_t shift;   // s - 1
};

DFN_RAYDIV_HD constexpr RayDiv ray_div_of(uint32_t n) {
  if (n <= 1) return RayDiv{0u, 0u};
  uint32_t s = 0;
  while ((uint64_t(1) << s) < n) ++s;   // s = ceil(log2 n), 1 .. 32
  const uint64_t p = uint64_t(1) << (31 + s);
  return RayDiv{uint32_t((p + n - 1) / n), s - 1};
}

DFN_RAYDIV_HD constexpr uint32_t umulhi32(uint32_t a, uint32_t b) { return uint32_t((uint64_t(a) * b) >> 32); }

// q / n for q < 2^31, d = ray_div_of(n)
DFN_RAYDIV_HD constexpr uint32_t ray_div(uint32_t q, RayDiv d) { return d.magic ? umulhi32(q, d.magic) >> d.shift : q; }

}  // namespace dfn

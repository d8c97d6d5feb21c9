"""Point index -> ray index by multiply-high and shift (dfnet_amd/csrc/nerfh_raydiv.h, kernel variant 12) against the division it replaces.

No GPU: a stand-alone host program with its own main around the shared header, compiled here with the host compiler, checks
umulhi(q, m) >> shift == q / n for

  * every n in 1..512 (the render's bound on Nc + Ni),
  * every q in {k n - 1, k n, k n + 1} with k n stepping through [0, 2^31) (every multiple of n below 2^31: the points at which the
    quotient steps),
  * q in {0, 1, 2^31 - 1},
  * 10^6 seeded random q < 2^31 per n,

(the stepping takes its expected quotients k - 1, k, k without dividing -- they are q / n by the definition of a multiple -- so that
its 4e10 points run in seconds on up to 16 threads; the edge and random points divide)

and that magic and shift are the ones the header's comment derives (m = ceil(2^(31+s) / n) in 32 bits, shift = s - 1; magic 0 for
n = 1).  The kernels see q < 2^31 only (launch_tiles refuses larger launches).  The same program is built a second time with
-fsanitize=address,undefined and run as it is: it needs no preloaded runtime.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dfnet_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

PROGRAM = r"""
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>
#include "nerfh_raydiv.h"

static std::atomic<uint64_t> bad{0}, checked{0};
static std::atomic<uint32_t> next_n{1};
static void report(uint32_t q, uint32_t n, uint32_t got, uint32_t want) {
  if (bad++ < 10) std::printf("q %u n %u: %u, expected %u\n", q, n, got, want);
}

static void worker(const std::vector<uint32_t>* rnd) {
  const uint64_t lim = 1ull << 31;
  for (uint32_t n; (n = next_n++) <= 512;) {
    const dfn::RayDiv d = dfn::ray_div_of(n);
    uint64_t cnt = 0;
    if (n == 1) {
      if (d.magic != 0) report(0, 1, d.magic, 0);
    } else {
      uint32_t sh = 0;
      while ((1ull << sh) < n) ++sh;
      const uint64_t m = ((1ull << (31 + sh)) + n - 1) / n;
      if (m >> 32 || m < (1ull << 31) || d.magic != uint32_t(m) || d.shift != sh - 1) report(0, n, d.magic, uint32_t(m));
    }
    // q = k n - 1, k n, k n + 1 for every multiple k n < 2^31.  Their quotients need no division: k n / n = k, and for n >= 2
    // (k n - 1) / n = k - 1 and (k n + 1) / n = k; for n = 1 the three are k - 1, k, k + 1.
    const uint32_t up = n == 1 ? 1u : 0u;
    uint32_t k = 0;
    for (uint64_t kn = 0; kn < lim; kn += n, ++k) {
      const uint32_t q = uint32_t(kn);
      if (dfn::ray_div(q, d) != k) report(q, n, dfn::ray_div(q, d), k);
      if (kn > 0 && dfn::ray_div(q - 1, d) != k - 1) report(q - 1, n, dfn::ray_div(q - 1, d), k - 1);
      if (kn + 1 < lim && dfn::ray_div(q + 1, d) != k + up) report(q + 1, n, dfn::ray_div(q + 1, d), k + up);
      cnt += 3;
    }
    const uint32_t edge[3] = {0u, 1u, uint32_t(lim - 1)};
    for (uint32_t q : edge)
      if (dfn::ray_div(q, d) != q / n) report(q, n, dfn::ray_div(q, d), q / n);
    for (uint32_t q : *rnd)
      if (dfn::ray_div(q, d) != q / n) report(q, n, dfn::ray_div(q, d), q / n);
    checked += cnt + 3 + rnd->size();
  }
}

int main() {
  std::vector<uint32_t> rnd(1000000);
  uint64_t s = 0x9e3779b97f4a7c15ull;   // xorshift64*, seeded
  for (auto& r : rnd) {
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    r = uint32_t((s * 0x2545f4914f6cdd1dull) >> 33);   // 31 bits
  }
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < nt; ++t) pool.emplace_back(worker, &rnd);
  for (auto& t : pool) t.join();
  std::printf("checked %llu bad %llu\n", (unsigned long long)checked.load(), (unsigned long long)bad.load());
  return bad.load() ? 1 : 0;
}
"""


def _build_and_run(tmp, name, *flags):
    src, exe = os.path.join(tmp, "ray_div_main.cpp"), os.path.join(tmp, name)
    with open(src, "w") as f:
        f.write(PROGRAM)
    p = subprocess.run([CXX, "-std=c++17", "-O2", "-pthread", *flags, "-I", CSRC, src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert " bad 0" in r.stdout
    return r.stdout


def test_magic_division_is_exact_below_2_31(tmp_path):
    out = _build_and_run(str(tmp_path), "ray_div")
    assert int(out.split("checked ")[1].split()[0]) > 512 * 10 ** 6


def test_magic_division_under_address_and_undefined_sanitizers(tmp_path):
    # the sanitizer runtimes linked statically: the program then starts whatever else the environment loads in front of it
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(CXX) and "clang" not in os.path.basename(CXX) else []
    _build_and_run(str(tmp_path), "ray_div_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", *static)
